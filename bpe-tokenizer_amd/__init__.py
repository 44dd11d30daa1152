"""bpe-tokenizer_amd — MI355X-native engine for the BPE merge-training hot path of
beenotung/bpe-tokenizer (reference: core.ts findNextMerge/applyMerge/mergeUntil).

This module is the Python (ctypes) binding of libbpe.so (C ABI: include/bpe.h).  The drop-in
replacement of the reference's `BPETokenizer` class lives in js/core.js (Node N-API addon over the
same C ABI); this binding serves the bench, the tests and multi-process (one rank per GPU) runs.

There is no CPU fallback: importing works anywhere (so the C ABI can be inspected), but creating
an `Engine` requires libbpe.so and a HIP device and raises otherwise.

Import with ``importlib.import_module('bpe-tokenizer_amd')`` (the directory name has a hyphen).
"""
import ctypes
import os
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
# BPE_LIB selects an experimental build of the same C ABI (tools/ kernel experiments)
LIB_PATH = os.environ.get('BPE_LIB') or os.path.join(HERE, 'libbpe.so')

BPE_OK = 0
BPE_NO_MERGE = 1
MAX_VOCAB = 55296

# Every symbol include/bpe.h and include/bpe_tools.h declare (checked by tests/test_capi.py).
C_API = [
    'bpe_version', 'bpe_last_error', 'bpe_device_count', 'bpe_create', 'bpe_destroy',
    'bpe_create_multi', 'bpe_shard_count', 'bpe_set_mode',
    'bpe_set_token_len16', 'bpe_num_tokens', 'bpe_add_sample', 'bpe_add_latin1',
    'bpe_clear_corpus', 'bpe_corpus_size', 'bpe_read_corpus', 'bpe_sample_lengths',
    'bpe_read_samples', 'bpe_find_next_merge',
    'bpe_apply_merge', 'bpe_apply_merges', 'bpe_merge_until', 'bpe_stats_enable', 'bpe_get_stats', 'bpe_reset_stats',
    'bpe_get_stream', 'bpe_synth_latin1', 'bpe_synth_zipf', 'bpe_recount', 'bpe_export_counts',
    'bpe_debug_tables', 'bpe_table_state', 'bpe_debug_tables_shard', 'bpe_debug_global',
    'bpe_debug_pix', 'bpe_debug_pix_shard', 'bpe_debug_pix_hook',
    'bpe_digest',
    'bpe_heavy_counts', 'bpe_select_counts', 'bpe_tie_positions', 'bpe_rank_loop_begin',
    'bpe_rank_loop_select', 'bpe_rank_loop_decide', 'bpe_rank_loop_count', 'bpe_rank_loop_end',
    'bpe_cold_counts', 'bpe_set_global_counts',
    'bpe_encoder_create', 'bpe_encoder_destroy', 'bpe_encoder_add_merges', 'bpe_encoder_clear',
    'bpe_encoder_num_merges', 'bpe_encode_batch', 'bpe_encoder_get_stats', 'bpe_encoder_reset_stats',
    'bpe_rccl_unique_id', 'bpe_rank_rccl_init', 'bpe_rank_loop_rccl', 'bpe_rank_rccl_destroy',
    'bpe_decoder_create', 'bpe_decoder_destroy', 'bpe_decoder_clear', 'bpe_decoder_add_tokens',
    'bpe_decoder_add_merges', 'bpe_decoder_num_tokens', 'bpe_decoder_set_vector_index',
    'bpe_decode_batch', 'bpe_decode_batch_device', 'bpe_decoder_get_stats', 'bpe_decoder_reset_stats',
    'bpe_encoder_set_chars', 'bpe_encoder_set_vector_index', 'bpe_encode_text_batch',
    'bpe_encode_text_batch_device', 'bpe_encoder_get_text_stats', 'bpe_encoder_reset_text_stats',
    'bpe_set_chars', 'bpe_add_text_batch', 'bpe_add_text_batch_device', 'bpe_get_ingest_stats',
    'bpe_reset_ingest_stats',
    'bpe_encoder_set_long_texts', 'bpe_encoder_get_split_stats', 'bpe_encoder_reset_split_stats',
    'bpe_add_sample_batch', 'bpe_add_sample_batch_device', 'bpe_restore_text_batch',
    'bpe_restore_text_batch_device', 'bpe_token_counts', 'bpe_get_append_stats', 'bpe_reset_append_stats',
    'bpe_export_samples', 'bpe_export_samples_device', 'bpe_export_text_batch', 'bpe_export_text_batch_device',
    'bpe_get_export_stats', 'bpe_reset_export_stats',
    'bpe_encoder_utf8_to_utf16', 'bpe_encoder_utf8_to_utf16_device', 'bpe_encode_utf8_batch',
    'bpe_encode_utf8_batch_device', 'bpe_add_utf8_batch', 'bpe_add_utf8_batch_device', 'bpe_restore_utf8_batch',
    'bpe_restore_utf8_batch_device', 'bpe_encoder_get_utf8_stats', 'bpe_encoder_reset_utf8_stats',
    'bpe_get_utf8_stats', 'bpe_reset_utf8_stats',
    'bpe_decoder_utf16_to_utf8', 'bpe_decoder_utf16_to_utf8_device', 'bpe_decode_utf8_batch',
    'bpe_decode_utf8_batch_device', 'bpe_export_utf8_batch', 'bpe_export_utf8_batch_device',
    'bpe_decoder_get_utf8_stats', 'bpe_decoder_reset_utf8_stats',
    'bpe_encoder_split_lines', 'bpe_encoder_split_lines_device', 'bpe_add_lines_batch', 'bpe_add_lines_batch_device',
    'bpe_add_lines_utf8_batch', 'bpe_add_lines_utf8_batch_device', 'bpe_restore_lines_batch',
    'bpe_restore_lines_batch_device', 'bpe_restore_lines_utf8_batch', 'bpe_restore_lines_utf8_batch_device',
    'bpe_encoder_get_lines_stats', 'bpe_encoder_reset_lines_stats', 'bpe_get_lines_stats', 'bpe_reset_lines_stats',
    'bpe_encoder_skipgram', 'bpe_encoder_skipgram_device', 'bpe_skipgram_text_batch', 'bpe_skipgram_text_batch_device',
    'bpe_skipgram_utf8_batch', 'bpe_skipgram_utf8_batch_device', 'bpe_export_skipgram', 'bpe_export_skipgram_device',
    'bpe_encoder_get_skipgram_stats', 'bpe_encoder_reset_skipgram_stats', 'bpe_get_skipgram_stats',
    'bpe_reset_skipgram_stats',
]
HOT_BINS = 65536
# bpe_debug_global (include/bpe_tools.h): the info words in order (BPE_GLOBAL_INFO_*)
GLOBAL_INFO = ['held', 'pending', 'a', 'b', 'c', 'w', 'multi_maintained', 'xchg_words']
# bpe_debug_pix (include/bpe_tools.h): the info words in order (BPE_PIX_INFO_*), and the arrays in
# order with their element types and which info word sizes them
PIX_INFO_WORDS = 24
PIX_INFO = ['present', 'n', 'cap', 'nblocks', 'nsuper', 'ml', 'status', 'tie', 'err', 'used', 'used_cap',
            'pool_top', 'pool_cap', 'n_dblocks', 'n_dsuper', 'next_id', 'merged', 'n_done', 'sharded',
            'delta_pending', 'pair_slot', 'max_id']
PIX_ARRAYS = [('tok', np.int32, 'n'), ('nxt', np.uint32, 'n'), ('prv', np.uint32, 'n'),
              ('keys', np.uint32, 'cap'), ('cnt', np.uint64, 'cap'), ('off', np.uint32, 'cap'),
              ('len', np.uint32, 'cap'), ('fill', np.uint32, 'cap'), ('bmax', np.uint64, 'nblocks'),
              ('sbmax', np.uint64, 'nsuper'), ('bdirty', np.uint32, 'nblocks'),
              ('sbdirty', np.uint32, 'nsuper'), ('pool', np.uint32, 'pool_top'),
              ('dblocks', np.uint32, 'n_dblocks'), ('dsuper', np.uint32, 'n_dsuper')]
PIX_HOOK = ctypes.CFUNCTYPE(None, ctypes.c_void_p, ctypes.c_int)
PIX_RUN, PIX_DONE, PIX_HOST, PIX_ERROR, PIX_PAUSE = range(5)          # PixStatus
PIX_TIE_NONE, PIX_TIE_SCAN, PIX_TIE_DECIDED, PIX_TIE_WAIT = range(4)  # PixTie
TABLE_BINS = 81920
DIGEST_MOD = 254    # BPE_DIGEST_MOD: the digest plane's code of a token id t >= 0 is t % DIGEST_MOD
DIGEST_SEP = 254    # BPE_DIGEST_SEP: ... of a sample separator (-1)
DIGEST_DEAD = 255   # BPE_DIGEST_DEAD: ... of a dead slot (anything below -1)
DIGEST_CAND = 8     # BPE_DIGEST_CAND: candidate pairs one stream of the plane answers for
MAX_CAND = 16       # BPE_MAX_CAND
REDUCE_RCCL = 0     # BPE_REDUCE_RCCL
REDUCE_HOST = 1     # BPE_REDUCE_HOST
MODE_STREAM = 0     # BPE_MODE_STREAM
MODE_INCREMENTAL = 1   # BPE_MODE_INCREMENTAL
LOOP_BATCH = 64     # BPE_LOOP_BATCH
XCHG_HDR = 8        # BPE_XCHG_HDR
DELTA_ROWS = 6      # BPE_DELTA_ROWS
XCHG_WORDS = XCHG_HDR + DELTA_ROWS * MAX_VOCAB   # BPE_XCHG_WORDS
TIE_WORDS = 32      # BPE_TIE_WORDS
ENCODE_LDS_TOKENS = 16384   # BPE_ENCODE_LDS_TOKENS: longer texts are replayed by apply passes, or split
LONG_REPLAY = 0     # BPE_LONG_REPLAY: long texts are replayed (the default)
LONG_SPLIT = 1      # BPE_LONG_SPLIT: long texts are cut at boundaries no merge can cross
ENCODE_SPLIT_WINDOW = 1024  # BPE_ENCODE_SPLIT_WINDOW: boundaries per window of the cut search
DECODE_TILE = 1024  # BPE_DECODE_TILE: values per workgroup of the decode kernels
DECODE_SCAN_ROUND = 8192   # BPE_DECODE_SCAN_ROUND: tile sums per round of the decode kernels' scan
DECODE_IDS = 0      # BPE_DECODE_IDS: decodeTokens, values are token ids
DECODE_VECTORS = 1  # BPE_DECODE_VECTORS: decodeVector, values are vector indices
TEXT_TILE = 2048    # BPE_TEXT_TILE: UTF-16 units per workgroup of the text front end
TEXT_SCAN_ROUND = 2048   # BPE_TEXT_SCAN_ROUND: tile counts per round of the front end's scan
ENCODE_IDS = 0      # BPE_ENCODE_IDS: text -> token ids
ENCODE_VECTORS = 1  # BPE_ENCODE_VECTORS: text -> vector indices (encodeToVector)
APPEND_TILE = 2048  # BPE_APPEND_TILE: corpus slots per tile of the append kernel
EXPORT_TILE = 256   # BPE_EXPORT_TILE: corpus slots per wave step of the export kernels
EXPORT_SCAN_THREADS = 1024   # BPE_EXPORT_SCAN_THREADS: threads of the one-block scan of the export's prefixes
EXPORT_IDS = 0      # BPE_EXPORT_IDS: samples out as token ids
EXPORT_VECTORS = 1  # BPE_EXPORT_VECTORS: ... as vector indices (encodeToVector of every sample)
EXPORT_CODE = 2     # BPE_EXPORT_CODE: ... as uint16 code units id + 1 (corpus_in_code)
UTF8_TILE = 4096    # BPE_UTF8_TILE: bytes per workgroup of the UTF-8 transcode (its scan round: TEXT_SCAN_ROUND)
UTF16_TILE = 2048   # BPE_UTF16_TILE: units per workgroup of the transcode to UTF-8 (the same scan round)
LINES_TRIM = 0      # BPE_LINES_TRIM: linesToCorpus (cut at LF, trim(), wrapped in CR .. LF)
LINES_KEEP = 1      # BPE_LINES_KEEP: linesTrimmedToCorpus (cut at LF, one trailing CR dropped, the same wrap)
LINES_FILE = 2      # BPE_LINES_FILE: fileContentToCorpus (U+001C + text + U+0004)
SKIPGRAM_MAX_WINDOW = 64    # BPE_SKIPGRAM_MAX_WINDOW: the widest window of the skip-gram expansion
SKIPGRAM_TILE = 2048        # BPE_SKIPGRAM_TILE: pairs per workgroup of the expand kernel
SKIPGRAM_SCAN_ROUND = 8192  # BPE_SKIPGRAM_SCAN_ROUND: texts per round of the scan of the pair counts
_LINES_MODES = {'trim': LINES_TRIM, 'keep': LINES_KEEP, 'file': LINES_FILE,
                LINES_TRIM: LINES_TRIM, LINES_KEEP: LINES_KEEP, LINES_FILE: LINES_FILE}


ERR_ARG, ERR_HIP, ERR_OOM, ERR_STATE, ERR_VOCAB = -1, -2, -3, -4, -5
ERR_NOFIT = -6      # BPE_ERR_NOFIT: the position index does not fit beside the shard's corpus


class BpeError(RuntimeError):
    """A libbpe call failed; `code` is its status (BPE_ERR_*, include/bpe.h)."""

    def __init__(self, msg, code=None):
        super().__init__(msg)
        self.code = code


class Stats(ctypes.Structure):
    _fields_ = [
        ('step_ms', ctypes.c_double), ('step_launches', ctypes.c_int64),
        ('step_slots', ctypes.c_int64), ('step_live', ctypes.c_int64),
        ('select_ms', ctypes.c_double), ('tie_passes', ctypes.c_int64),
        ('iterations', ctypes.c_int64), ('live_tokens', ctypes.c_int64),
        ('compactions', ctypes.c_int64), ('exact_passes', ctypes.c_int64),
        ('step_timed', ctypes.c_int64), ('tie_tail', ctypes.c_int64),
        ('tie_lone', ctypes.c_int64), ('loop_host', ctypes.c_int64),
        ('fused_passes', ctypes.c_int64), ('pix_builds', ctypes.c_int64),
        ('pix_merges', ctypes.c_int64), ('pix_host', ctypes.c_int64),
        ('pix_build_ms', ctypes.c_double), ('cold_used', ctypes.c_int64),
        ('sel_blocks', ctypes.c_int64), ('xchg_bytes', ctypes.c_int64),
        ('xchg_iters', ctypes.c_int64), ('pix_fallbacks', ctypes.c_int64),
        ('cold_rebuilds', ctypes.c_int64), ('incr_ms', ctypes.c_double),
        ('incr_timed', ctypes.c_int64), ('incr_launches', ctypes.c_int64),
        ('incr_live', ctypes.c_int64), ('unscreened_passes', ctypes.c_int64),
        ('delta_passes', ctypes.c_int64), ('delta_chunks', ctypes.c_int64),
        ('digest_passes', ctypes.c_int64), ('digest_hits', ctypes.c_int64),
        ('digest_builds', ctypes.c_int64), ('digest_scans', ctypes.c_int64),
    ]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


def rccl_unique_id():
    """ncclGetUniqueId of the RCCL beside libbpe's HIP runtime: 128 bytes (bpe_rccl_unique_id)."""
    buf = ctypes.create_string_buffer(128)
    _check(lib().bpe_rccl_unique_id(buf, 128), 'bpe_rccl_unique_id')
    return buf.raw


class EncoderStats(ctypes.Structure):
    """bpe_encoder_stats (include/bpe.h)."""
    _fields_ = [('kernel_ms', ctypes.c_double), ('calls', ctypes.c_int64),
                ('texts_rank', ctypes.c_int64), ('texts_replay', ctypes.c_int64),
                ('tokens_in', ctypes.c_int64), ('tokens_out', ctypes.c_int64),
                ('steps', ctypes.c_int64)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


class SplitStats(ctypes.Structure):
    """bpe_split_stats (include/bpe.h)."""
    _fields_ = [('calls', ctypes.c_int64), ('texts_split', ctypes.c_int64),
                ('texts_fallback', ctypes.c_int64), ('windows', ctypes.c_int64),
                ('segments', ctypes.c_int64), ('plan_ms', ctypes.c_double)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


class DecoderStats(ctypes.Structure):
    """bpe_decoder_stats (include/bpe.h)."""
    _fields_ = [('kernel_ms', ctypes.c_double), ('calls', ctypes.c_int64),
                ('texts', ctypes.c_int64), ('values_in', ctypes.c_int64),
                ('units_out', ctypes.c_int64)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


class TextStats(ctypes.Structure):
    """bpe_text_stats (include/bpe.h)."""
    _fields_ = [('calls', ctypes.c_int64), ('texts', ctypes.c_int64), ('units_in', ctypes.c_int64),
                ('chars', ctypes.c_int64), ('values_out', ctypes.c_int64),
                ('front_ms', ctypes.c_double), ('back_ms', ctypes.c_double)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


class IngestStats(ctypes.Structure):
    """bpe_ingest_stats (include/bpe.h)."""
    _fields_ = [('calls', ctypes.c_int64), ('texts', ctypes.c_int64), ('units', ctypes.c_int64),
                ('chars', ctypes.c_int64), ('new_chars', ctypes.c_int64), ('kernel_ms', ctypes.c_double)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


class AppendStats(ctypes.Structure):
    """bpe_append_stats (include/bpe.h)."""
    _fields_ = [('calls', ctypes.c_int64), ('samples', ctypes.c_int64), ('tokens', ctypes.c_int64),
                ('kernel_ms', ctypes.c_double)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


class ExportStats(ctypes.Structure):
    """bpe_export_stats (include/bpe.h)."""
    _fields_ = [('calls', ctypes.c_int64), ('samples', ctypes.c_int64), ('values', ctypes.c_int64),
                ('kernel_ms', ctypes.c_double)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


class Utf8Stats(ctypes.Structure):
    """bpe_utf8_stats (include/bpe.h)."""
    _fields_ = [('calls', ctypes.c_int64), ('texts', ctypes.c_int64), ('bytes', ctypes.c_int64),
                ('units', ctypes.c_int64), ('replaced', ctypes.c_int64), ('kernel_ms', ctypes.c_double)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


class LinesStats(ctypes.Structure):
    """bpe_lines_stats (include/bpe.h)."""
    _fields_ = [('calls', ctypes.c_int64), ('texts', ctypes.c_int64), ('units_in', ctypes.c_int64),
                ('samples', ctypes.c_int64), ('units_out', ctypes.c_int64), ('trimmed', ctypes.c_int64),
                ('kernel_ms', ctypes.c_double)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


class SkipgramStats(ctypes.Structure):
    """bpe_skipgram_stats (include/bpe.h)."""
    _fields_ = [('calls', ctypes.c_int64), ('texts', ctypes.c_int64), ('values_in', ctypes.c_int64),
                ('pairs_out', ctypes.c_int64), ('kernel_ms', ctypes.c_double)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


def build(force=False):
    """Compiles libbpe.so for gfx950 (hipcc cross-compiles; no GPU needed)."""
    if force or not os.path.exists(LIB_PATH):
        subprocess.check_call(['make', '-s', '-C', HERE] + (['-B'] if force else []))
    return LIB_PATH


_lib = None


def lib():
    """Loads libbpe.so (raises if it was not built — no fallback)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise BpeError('libbpe.so is missing: run make -C bpe-tokenizer_amd (HIP engine required)')
    L = ctypes.CDLL(LIB_PATH)
    i32p, i64p = ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_int64)
    vp = ctypes.c_void_p
    sig = {
        'bpe_version': ([], ctypes.c_int),
        'bpe_last_error': ([ctypes.c_char_p, ctypes.c_size_t], ctypes.c_int),
        'bpe_device_count': ([ctypes.POINTER(ctypes.c_int)], ctypes.c_int),
        'bpe_create': ([ctypes.POINTER(vp), ctypes.c_int], ctypes.c_int),
        'bpe_destroy': ([vp], ctypes.c_int),
        'bpe_create_multi': ([ctypes.POINTER(vp), ctypes.c_int, ctypes.POINTER(ctypes.c_int),
                              ctypes.c_int], ctypes.c_int),
        'bpe_shard_count': ([vp, ctypes.POINTER(ctypes.c_int)], ctypes.c_int),
        'bpe_set_mode': ([vp, ctypes.c_int], ctypes.c_int),
        'bpe_set_token_len16': ([vp, ctypes.c_int32, ctypes.c_int32], ctypes.c_int),
        'bpe_num_tokens': ([vp, i32p], ctypes.c_int),
        'bpe_add_sample': ([vp, i32p, ctypes.c_int64], ctypes.c_int),
        'bpe_add_latin1': ([vp, ctypes.c_void_p, ctypes.c_int64, ctypes.c_int64, i32p, i32p, i64p],
                           ctypes.c_int),
        'bpe_clear_corpus': ([vp], ctypes.c_int),
        'bpe_corpus_size': ([vp, i64p, i64p], ctypes.c_int),
        'bpe_read_corpus': ([vp, i32p, ctypes.c_int64, i64p, ctypes.c_int64], ctypes.c_int),
        'bpe_sample_lengths': ([vp, i64p, ctypes.c_int64], ctypes.c_int),
        'bpe_read_samples': ([vp, i64p, ctypes.c_int64, i32p, ctypes.c_int64, i64p], ctypes.c_int),
        'bpe_find_next_merge': ([vp, ctypes.c_int64, ctypes.c_int64, i32p, i32p, i64p],
                                ctypes.c_int),
        'bpe_apply_merge': ([vp, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, i64p],
                            ctypes.c_int),
        'bpe_apply_merges': ([vp, i32p, ctypes.c_int64, i64p, ctypes.c_int], ctypes.c_int),
        'bpe_merge_until': ([vp, ctypes.c_int64, ctypes.c_int64, ctypes.c_int64, i64p,
                             ctypes.c_int64, i64p], ctypes.c_int),
        'bpe_stats_enable': ([vp, ctypes.c_int], ctypes.c_int),
        'bpe_get_stats': ([vp, ctypes.POINTER(Stats)], ctypes.c_int),
        'bpe_reset_stats': ([vp], ctypes.c_int),
        'bpe_get_stream': ([vp, ctypes.POINTER(vp)], ctypes.c_int),
        'bpe_recount': ([vp], ctypes.c_int),
        'bpe_debug_tables': ([vp, vp, vp, vp, ctypes.c_int64, i64p], ctypes.c_int),
        'bpe_table_state': ([vp, ctypes.POINTER(ctypes.c_int)], ctypes.c_int),
        'bpe_debug_tables_shard': ([vp, ctypes.c_int, vp, vp, vp, ctypes.c_int64, i64p], ctypes.c_int),
        'bpe_debug_global': ([vp, ctypes.c_int, i64p, vp, ctypes.c_int64], ctypes.c_int),
        'bpe_debug_pix': ([vp, i64p, vp], ctypes.c_int),
        'bpe_debug_pix_shard': ([vp, ctypes.c_int, i64p, vp], ctypes.c_int),
        'bpe_debug_pix_hook': ([vp, PIX_HOOK, vp, ctypes.c_int64], ctypes.c_int),
        'bpe_export_counts': ([vp, vp], ctypes.c_int),
        'bpe_heavy_counts': ([vp, vp, ctypes.c_int64, vp, vp, ctypes.c_int64, i64p], ctypes.c_int),
        'bpe_select_counts': ([vp, vp, vp, vp, ctypes.c_int64, ctypes.c_int64, ctypes.c_int64,
                               i32p, ctypes.c_int64, i64p, i64p], ctypes.c_int),
        'bpe_tie_positions': ([vp, i32p, ctypes.c_int64, ctypes.POINTER(ctypes.c_uint64)],
                              ctypes.c_int),
        'bpe_rank_loop_begin': ([vp, ctypes.c_int64, ctypes.c_int64, vp, vp, ctypes.c_int,
                                 ctypes.c_int, i64p], ctypes.c_int),
        'bpe_cold_counts': ([vp, vp, vp, ctypes.c_int64, i64p], ctypes.c_int),
        'bpe_set_global_counts': ([vp, vp, vp, vp, ctypes.c_int64], ctypes.c_int),
        'bpe_rank_loop_select': ([vp], ctypes.c_int),
        'bpe_rank_loop_decide': ([vp], ctypes.c_int),
        'bpe_rank_loop_count': ([vp], ctypes.c_int),
        'bpe_rank_loop_end': ([vp, i64p, ctypes.c_int64, i64p, ctypes.POINTER(ctypes.c_int)],
                              ctypes.c_int),
        'bpe_rccl_unique_id': ([vp, ctypes.c_size_t], ctypes.c_int),
        'bpe_rank_rccl_init': ([vp, vp, ctypes.c_int, ctypes.c_int], ctypes.c_int),
        'bpe_rank_loop_rccl': ([vp, vp, ctypes.c_int64, vp, ctypes.c_int], ctypes.c_int),
        'bpe_rank_rccl_destroy': ([vp], ctypes.c_int),
        'bpe_encoder_create': ([ctypes.POINTER(vp), ctypes.c_int], ctypes.c_int),
        'bpe_encoder_destroy': ([vp], ctypes.c_int),
        'bpe_encoder_add_merges': ([vp, i32p, ctypes.c_int64], ctypes.c_int),
        'bpe_encoder_clear': ([vp], ctypes.c_int),
        'bpe_encoder_num_merges': ([vp, i64p], ctypes.c_int),
        'bpe_encode_batch': ([vp, i32p, i64p, ctypes.c_int64, i32p, i64p], ctypes.c_int),
        'bpe_encoder_get_stats': ([vp, ctypes.POINTER(EncoderStats)], ctypes.c_int),
        'bpe_encoder_reset_stats': ([vp], ctypes.c_int),
        'bpe_encoder_set_long_texts': ([vp, ctypes.c_int], ctypes.c_int),
        'bpe_encoder_get_split_stats': ([vp, ctypes.POINTER(SplitStats)], ctypes.c_int),
        'bpe_encoder_reset_split_stats': ([vp], ctypes.c_int),
        'bpe_decoder_create': ([ctypes.POINTER(vp), ctypes.c_int], ctypes.c_int),
        'bpe_decoder_destroy': ([vp], ctypes.c_int),
        'bpe_decoder_clear': ([vp], ctypes.c_int),
        'bpe_decoder_add_tokens': ([vp, vp, i64p, ctypes.c_int64], ctypes.c_int),
        'bpe_decoder_add_merges': ([vp, i32p, ctypes.c_int64], ctypes.c_int),
        'bpe_decoder_num_tokens': ([vp, i32p, i64p], ctypes.c_int),
        'bpe_decoder_set_vector_index': ([vp, i32p, ctypes.c_int32], ctypes.c_int),
        'bpe_decode_batch': ([vp, ctypes.c_int, i32p, i64p, ctypes.c_int64, vp, ctypes.c_int64, i64p],
                             ctypes.c_int),
        'bpe_decode_batch_device': ([vp, ctypes.c_int, vp, vp, ctypes.c_int64, vp, ctypes.c_int64, vp,
                                     i64p], ctypes.c_int),
        'bpe_decoder_get_stats': ([vp, ctypes.POINTER(DecoderStats)], ctypes.c_int),
        'bpe_decoder_reset_stats': ([vp], ctypes.c_int),
        'bpe_encoder_set_chars': ([vp, vp, i32p, ctypes.c_int64], ctypes.c_int),
        'bpe_encoder_set_vector_index': ([vp, i32p, ctypes.c_int32], ctypes.c_int),
        'bpe_encode_text_batch': ([vp, ctypes.c_int, vp, i64p, ctypes.c_int64, vp, ctypes.c_int64, i64p],
                                  ctypes.c_int),
        'bpe_encode_text_batch_device': ([vp, ctypes.c_int, vp, vp, ctypes.c_int64, vp, ctypes.c_int64, vp,
                                          i64p], ctypes.c_int),
        'bpe_encoder_get_text_stats': ([vp, ctypes.POINTER(TextStats)], ctypes.c_int),
        'bpe_encoder_reset_text_stats': ([vp], ctypes.c_int),
        'bpe_set_chars': ([vp, vp, i32p, ctypes.c_int64], ctypes.c_int),
        'bpe_add_text_batch': ([vp, vp, i64p, ctypes.c_int64, vp, ctypes.c_int64, i64p, i64p, ctypes.c_int64],
                               ctypes.c_int),
        'bpe_add_text_batch_device': ([vp, vp, vp, ctypes.c_int64, vp, ctypes.c_int64, i64p, i64p,
                                       ctypes.c_int64], ctypes.c_int),
        'bpe_get_ingest_stats': ([vp, ctypes.POINTER(IngestStats)], ctypes.c_int),
        'bpe_reset_ingest_stats': ([vp], ctypes.c_int),
        'bpe_add_sample_batch': ([vp, vp, i64p, ctypes.c_int64], ctypes.c_int),
        'bpe_add_sample_batch_device': ([vp, vp, vp, ctypes.c_int64], ctypes.c_int),
        'bpe_restore_text_batch': ([vp, vp, vp, i64p, ctypes.c_int64], ctypes.c_int),
        'bpe_restore_text_batch_device': ([vp, vp, vp, vp, ctypes.c_int64], ctypes.c_int),
        'bpe_token_counts': ([vp, i64p, ctypes.c_int64], ctypes.c_int),
        'bpe_get_append_stats': ([vp, ctypes.POINTER(AppendStats)], ctypes.c_int),
        'bpe_reset_append_stats': ([vp], ctypes.c_int),
        'bpe_export_samples': ([vp, ctypes.c_int, i64p, ctypes.c_int64, i32p, ctypes.c_int32, vp, ctypes.c_int64,
                                i64p], ctypes.c_int),
        'bpe_export_samples_device': ([vp, ctypes.c_int, i64p, ctypes.c_int64, i32p, ctypes.c_int32, vp,
                                       ctypes.c_int64, vp, i64p], ctypes.c_int),
        'bpe_export_text_batch': ([vp, vp, i64p, ctypes.c_int64, vp, ctypes.c_int64, i64p], ctypes.c_int),
        'bpe_export_text_batch_device': ([vp, vp, i64p, ctypes.c_int64, vp, ctypes.c_int64, vp, i64p],
                                         ctypes.c_int),
        'bpe_get_export_stats': ([vp, ctypes.POINTER(ExportStats)], ctypes.c_int),
        'bpe_reset_export_stats': ([vp], ctypes.c_int),
        'bpe_encoder_utf8_to_utf16': ([vp, vp, i64p, ctypes.c_int64, vp, ctypes.c_int64, i64p], ctypes.c_int),
        'bpe_encoder_utf8_to_utf16_device': ([vp, vp, vp, ctypes.c_int64, vp, ctypes.c_int64, vp, i64p],
                                             ctypes.c_int),
        'bpe_encode_utf8_batch': ([vp, ctypes.c_int, vp, i64p, ctypes.c_int64, vp, ctypes.c_int64, i64p],
                                  ctypes.c_int),
        'bpe_encode_utf8_batch_device': ([vp, ctypes.c_int, vp, vp, ctypes.c_int64, vp, ctypes.c_int64, vp,
                                          i64p], ctypes.c_int),
        'bpe_add_utf8_batch': ([vp, vp, i64p, ctypes.c_int64, vp, ctypes.c_int64, i64p, i64p, ctypes.c_int64],
                               ctypes.c_int),
        'bpe_add_utf8_batch_device': ([vp, vp, vp, ctypes.c_int64, vp, ctypes.c_int64, i64p, i64p,
                                       ctypes.c_int64], ctypes.c_int),
        'bpe_restore_utf8_batch': ([vp, vp, vp, i64p, ctypes.c_int64], ctypes.c_int),
        'bpe_restore_utf8_batch_device': ([vp, vp, vp, vp, ctypes.c_int64], ctypes.c_int),
        'bpe_encoder_get_utf8_stats': ([vp, ctypes.POINTER(Utf8Stats)], ctypes.c_int),
        'bpe_encoder_reset_utf8_stats': ([vp], ctypes.c_int),
        'bpe_get_utf8_stats': ([vp, ctypes.POINTER(Utf8Stats)], ctypes.c_int),
        'bpe_reset_utf8_stats': ([vp], ctypes.c_int),
        'bpe_decoder_utf16_to_utf8': ([vp, vp, i64p, ctypes.c_int64, vp, ctypes.c_int64, i64p], ctypes.c_int),
        'bpe_decoder_utf16_to_utf8_device': ([vp, vp, vp, ctypes.c_int64, vp, ctypes.c_int64, vp, i64p],
                                             ctypes.c_int),
        'bpe_decode_utf8_batch': ([vp, ctypes.c_int, i32p, i64p, ctypes.c_int64, vp, ctypes.c_int64, i64p],
                                  ctypes.c_int),
        'bpe_decode_utf8_batch_device': ([vp, ctypes.c_int, vp, vp, ctypes.c_int64, vp, ctypes.c_int64, vp,
                                          i64p], ctypes.c_int),
        'bpe_export_utf8_batch': ([vp, vp, i64p, ctypes.c_int64, vp, ctypes.c_int64, i64p], ctypes.c_int),
        'bpe_export_utf8_batch_device': ([vp, vp, i64p, ctypes.c_int64, vp, ctypes.c_int64, vp, i64p],
                                         ctypes.c_int),
        'bpe_decoder_get_utf8_stats': ([vp, ctypes.POINTER(Utf8Stats)], ctypes.c_int),
        'bpe_decoder_reset_utf8_stats': ([vp], ctypes.c_int),
        'bpe_encoder_split_lines': ([vp, ctypes.c_int, vp, i64p, ctypes.c_int64, vp, ctypes.c_int64, i64p,
                                     ctypes.c_int64, i64p], ctypes.c_int),
        'bpe_encoder_split_lines_device': ([vp, ctypes.c_int, vp, vp, ctypes.c_int64, vp, ctypes.c_int64, vp,
                                            ctypes.c_int64, i64p, i64p], ctypes.c_int),
        'bpe_add_lines_batch': ([vp, ctypes.c_int, vp, i64p, ctypes.c_int64, vp, ctypes.c_int64, i64p, i64p,
                                 ctypes.c_int64], ctypes.c_int),
        'bpe_add_lines_batch_device': ([vp, ctypes.c_int, vp, vp, ctypes.c_int64, vp, ctypes.c_int64, i64p, i64p,
                                        ctypes.c_int64], ctypes.c_int),
        'bpe_add_lines_utf8_batch': ([vp, ctypes.c_int, vp, i64p, ctypes.c_int64, vp, ctypes.c_int64, i64p, i64p,
                                      ctypes.c_int64], ctypes.c_int),
        'bpe_add_lines_utf8_batch_device': ([vp, ctypes.c_int, vp, vp, ctypes.c_int64, vp, ctypes.c_int64, i64p,
                                             i64p, ctypes.c_int64], ctypes.c_int),
        'bpe_restore_lines_batch': ([vp, vp, ctypes.c_int, vp, i64p, ctypes.c_int64], ctypes.c_int),
        'bpe_restore_lines_batch_device': ([vp, vp, ctypes.c_int, vp, vp, ctypes.c_int64], ctypes.c_int),
        'bpe_restore_lines_utf8_batch': ([vp, vp, ctypes.c_int, vp, i64p, ctypes.c_int64], ctypes.c_int),
        'bpe_restore_lines_utf8_batch_device': ([vp, vp, ctypes.c_int, vp, vp, ctypes.c_int64], ctypes.c_int),
        'bpe_encoder_get_lines_stats': ([vp, ctypes.POINTER(LinesStats)], ctypes.c_int),
        'bpe_encoder_reset_lines_stats': ([vp], ctypes.c_int),
        'bpe_get_lines_stats': ([vp, ctypes.POINTER(LinesStats)], ctypes.c_int),
        'bpe_reset_lines_stats': ([vp], ctypes.c_int),
        'bpe_encoder_skipgram': ([vp, vp, i64p, ctypes.c_int64, ctypes.c_int, vp, vp, ctypes.c_int64, i64p],
                                 ctypes.c_int),
        'bpe_encoder_skipgram_device': ([vp, vp, vp, ctypes.c_int64, ctypes.c_int, vp, vp, ctypes.c_int64, vp, i64p],
                                        ctypes.c_int),
        'bpe_skipgram_text_batch': ([vp, ctypes.c_int, vp, i64p, ctypes.c_int64, ctypes.c_int, vp, vp, ctypes.c_int64,
                                     i64p], ctypes.c_int),
        'bpe_skipgram_text_batch_device': ([vp, ctypes.c_int, vp, vp, ctypes.c_int64, ctypes.c_int, vp, vp,
                                            ctypes.c_int64, vp, i64p], ctypes.c_int),
        'bpe_skipgram_utf8_batch': ([vp, ctypes.c_int, vp, i64p, ctypes.c_int64, ctypes.c_int, vp, vp, ctypes.c_int64,
                                     i64p], ctypes.c_int),
        'bpe_skipgram_utf8_batch_device': ([vp, ctypes.c_int, vp, vp, ctypes.c_int64, ctypes.c_int, vp, vp,
                                            ctypes.c_int64, vp, i64p], ctypes.c_int),
        'bpe_export_skipgram': ([vp, ctypes.c_int, i64p, ctypes.c_int64, i32p, ctypes.c_int32, ctypes.c_int, vp, vp,
                                 ctypes.c_int64, i64p], ctypes.c_int),
        'bpe_export_skipgram_device': ([vp, ctypes.c_int, i64p, ctypes.c_int64, i32p, ctypes.c_int32, ctypes.c_int, vp,
                                        vp, ctypes.c_int64, vp, i64p], ctypes.c_int),
        'bpe_encoder_get_skipgram_stats': ([vp, ctypes.POINTER(SkipgramStats)], ctypes.c_int),
        'bpe_encoder_reset_skipgram_stats': ([vp], ctypes.c_int),
        'bpe_get_skipgram_stats': ([vp, ctypes.POINTER(SkipgramStats)], ctypes.c_int),
        'bpe_reset_skipgram_stats': ([vp], ctypes.c_int),
        'bpe_digest': ([i32p, ctypes.c_int64, ctypes.c_void_p], ctypes.c_int),
        'bpe_synth_zipf': ([ctypes.c_uint32, ctypes.c_double, ctypes.c_uint32, ctypes.c_uint64,
                            ctypes.c_int64, ctypes.c_void_p, ctypes.c_int64], ctypes.c_int),
        'bpe_synth_latin1': ([ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint64,
                              ctypes.c_void_p, ctypes.c_int64], ctypes.c_int),
    }
    for name, (args, res) in sig.items():
        if not hasattr(L, name):   # (an older experimental build: BPE_LIB)
            continue
        f = getattr(L, name)
        f.argtypes = args
        f.restype = res
    _lib = L
    return L


def last_error():
    buf = ctypes.create_string_buffer(1024)
    lib().bpe_last_error(buf, 1024)
    return buf.value.decode(errors='replace')


def _check(rc, what):
    if rc < 0:
        raise BpeError('%s failed (%d): %s' % (what, rc, last_error()), rc)
    return rc


def device_count():
    n = ctypes.c_int(0)
    _check(lib().bpe_device_count(ctypes.byref(n)), 'bpe_device_count')
    return n.value


def synth_latin1(n, seed=12345, A=256, base=0, skip=0):
    """SURVEY.md §8(d) synthetic corpus: xorshift32 bytes (jump-ahead `skip` outputs)."""
    out = np.empty(n, dtype=np.uint8)
    _check(lib().bpe_synth_latin1(seed, A, base, skip, out.ctypes.data, n), 'bpe_synth_latin1')
    return out


def synth_zipf(n, seed=12345, s=1.1, n_words=32768, sample_bytes=1 << 20, first_sample=0):
    """Skewed synthetic corpus (include/bpe_tools.h bpe_synth_zipf): Zipf(s) words from a fixed
    word list, samples of sample_bytes starting at sample `first_sample`."""
    out = np.empty(n, dtype=np.uint8)
    _check(lib().bpe_synth_zipf(seed, s, n_words, first_sample, sample_bytes, out.ctypes.data, n),
           'bpe_synth_zipf')
    return out


def _i32(a):
    return np.ascontiguousarray(a, dtype=np.int32)


def digest(ids):
    """The digest plane's byte of each slot value in `ids` (bpe_digest: the engine's own function;
    DIGEST_MOD, DIGEST_SEP and DIGEST_DEAD are its parameters)."""
    x = _i32(ids).ravel()
    out = np.empty(x.size, dtype=np.uint8)
    _check(lib().bpe_digest(x.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), x.size,
                            out.ctypes.data), 'bpe_digest')
    return out


class Engine:
    """One corpus shard on one HIP device (a `bpe_ctx`); with `devices`, one corpus sharded over
    several (bpe_create_multi: RCCL all-reduces, or host copies when reduce='host')."""

    def __init__(self, device=0, devices=None, reduce='rccl'):
        self._ctx = ctypes.c_void_p()
        self.device = int(device if devices is None else devices[0])
        if devices is None:
            _check(lib().bpe_create(ctypes.byref(self._ctx), device), 'bpe_create')
        else:
            dv = (ctypes.c_int * len(devices))(*devices)
            _check(lib().bpe_create_multi(ctypes.byref(self._ctx), len(devices), dv,
                                          REDUCE_HOST if reduce == 'host' else REDUCE_RCCL),
                   'bpe_create_multi')

    def set_mode(self, mode):
        """'stream' (every merge one pass over the corpus) or 'incremental' (mergeUntil on the
        position index: O(W) work per merge; bpe_set_mode)."""
        m = {'stream': MODE_STREAM, 'incremental': MODE_INCREMENTAL}[mode]
        _check(lib().bpe_set_mode(self._ctx, m), 'bpe_set_mode')

    def shard_count(self):
        n = ctypes.c_int()
        _check(lib().bpe_shard_count(self._ctx, ctypes.byref(n)), 'bpe_shard_count')
        return n.value

    def close(self):
        if self._ctx:
            lib().bpe_destroy(self._ctx)
            self._ctx = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # vocabulary -------------------------------------------------------------------------------
    def set_token_len16(self, token_id, len16):
        _check(lib().bpe_set_token_len16(self._ctx, token_id, len16), 'bpe_set_token_len16')

    def num_tokens(self):
        n = ctypes.c_int32()
        _check(lib().bpe_num_tokens(self._ctx, ctypes.byref(n)), 'bpe_num_tokens')
        return n.value

    # corpus ------------------------------------------------------------------------------------
    def add_sample(self, ids):
        a = _i32(ids)
        p = a.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)) if a.size else None
        _check(lib().bpe_add_sample(self._ctx, p, a.size), 'bpe_add_sample')

    def add_latin1(self, data, sample_bytes=0, char_to_id=None, n_tokens=None):
        """Bulk ingest; returns (char_to_id[256], n_tokens, char_hist[256])."""
        data = np.ascontiguousarray(np.frombuffer(data, dtype=np.uint8) if isinstance(data, (bytes, bytearray)) else data, dtype=np.uint8)
        cmap = np.full(256, -1, np.int32) if char_to_id is None else _i32(char_to_id).copy()
        nt = ctypes.c_int32(self.num_tokens() if n_tokens is None else n_tokens)
        hist = np.zeros(256, np.int64)
        _check(lib().bpe_add_latin1(self._ctx, data.ctypes.data, data.size, sample_bytes,
                                    cmap.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)),
                                    ctypes.byref(nt),
                                    hist.ctypes.data_as(ctypes.POINTER(ctypes.c_int64))),
               'bpe_add_latin1')
        return cmap, nt.value, hist

    # corpus from text: addToCorpus (core.ts:182-207) for batches of UTF-16 texts -------------------
    def set_chars(self, mapping):
        """Replaces the context's char table (char_to_token): a dict of a str of one code point (a
        lone surrogate included), or an int code point, to a token id.  An empty dict drops it."""
        cps = np.asarray([ord(k) if isinstance(k, str) else int(k) for k in mapping], dtype=np.uint32)
        ids = _i32(list(mapping.values()))
        cbuf = cps if cps.size else np.zeros(1, np.uint32)
        ibuf = ids if ids.size else np.zeros(1, np.int32)
        _check(lib().bpe_set_chars(self._ctx, cbuf.ctypes.data, ibuf.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)),
                                   cps.size), 'bpe_set_chars')

    def _add_text(self, fn, what, units_ptr, off_ptr, n, new_cap):
        """One call; a new_chars buffer that turns out too small is retried once with room."""
        hist = np.zeros(MAX_VOCAB, np.int64)
        n_new = ctypes.c_int64()
        for _ in range(2):
            new = np.zeros(max(new_cap, 1), np.uint32)
            rc = fn(self._ctx, units_ptr, off_ptr, n, new.ctypes.data, new_cap, ctypes.byref(n_new),
                    hist.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)), MAX_VOCAB)
            if rc == ERR_ARG and n_new.value > new_cap:
                new_cap = n_new.value
                continue
            break
        _check(rc, what)
        return new[:n_new.value].copy(), hist[:self.num_tokens()].copy()

    def add_text_flat(self, units, off, new_cap=1024):
        """Flat form (bpe_add_text_batch): texts units[off[k]:off[k+1]] (UTF-16 units), each one
        sample -> (new_chars uint32: the code point of every char token the call created, in id
        order from the token count before it; hist int64: this call's occurrences per token id)."""
        units = np.ascontiguousarray(units, dtype=np.uint16).ravel()
        off = np.ascontiguousarray(off, dtype=np.int64)
        src = units if units.size else np.zeros(1, np.uint16)
        return self._add_text(lib().bpe_add_text_batch, 'bpe_add_text_batch', src.ctypes.data,
                              off.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)), len(off) - 1, new_cap)

    def add_text(self, texts, new_cap=1024):
        """texts: a list of str (encoded with surrogatepass: lone surrogates survive) -> (new_chars, hist)."""
        parts = [_units(t) for t in texts]
        off = np.zeros(len(parts) + 1, dtype=np.int64)
        np.cumsum([len(x) for x in parts], out=off[1:])
        units = np.concatenate(parts).astype(np.uint16) if parts and off[-1] else np.zeros(0, np.uint16)
        return self.add_text_flat(units, off, new_cap)

    def add_text_tensors(self, units, off, new_cap=1024):
        """Device form (bpe_add_text_batch_device): units a torch int16 or uint16 tensor and off a
        torch int64 tensor on the context's device -> (new_chars, hist) as numpy arrays."""
        import torch
        if units.dtype not in (torch.int16, getattr(torch, 'uint16', torch.int16)) or off.dtype != torch.int64:
            raise BpeError('add_text_tensors takes int16 or uint16 units and int64 offsets', ERR_ARG)
        if not (units.is_cuda and off.is_cuda and units.device == off.device):
            raise BpeError('add_text_tensors takes tensors on the context\'s device', ERR_ARG)
        units, off = units.contiguous(), off.contiguous()
        torch.cuda.synchronize(units.device)   # (the context runs on a stream of its own)
        up = units.data_ptr() if units.numel() else None
        return self._add_text(lib().bpe_add_text_batch_device, 'bpe_add_text_batch_device', up,
                              off.data_ptr(), off.numel() - 1, new_cap)

    def ingest_stats(self):
        s = IngestStats()
        _check(lib().bpe_get_ingest_stats(self._ctx, ctypes.byref(s)), 'bpe_get_ingest_stats')
        return s.as_dict()

    def reset_ingest_stats(self):
        _check(lib().bpe_reset_ingest_stats(self._ctx), 'bpe_reset_ingest_stats')

    # corpus from encoded samples, and restoreToCorpus (core.ts:213-216) for batches of texts ----------
    def add_samples_flat(self, ids, off):
        """Flat form (bpe_add_sample_batch): sample k is ids[off[k]:off[k+1]]; the context ends up as
        after add_sample(sample) for each of them, and a failed call changes nothing."""
        ids = _i32(ids).ravel()
        off = np.ascontiguousarray(off, dtype=np.int64)
        src = ids if ids.size else np.zeros(1, np.int32)
        _check(lib().bpe_add_sample_batch(self._ctx, src.ctypes.data,
                                          off.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)), len(off) - 1),
               'bpe_add_sample_batch')

    def add_samples(self, samples):
        """samples: a list of id lists, each one sample."""
        off = np.zeros(len(samples) + 1, dtype=np.int64)
        np.cumsum([len(x) for x in samples], out=off[1:])
        ids = np.concatenate([_i32(x).ravel() for x in samples]) if len(samples) and off[-1] else np.zeros(0, np.int32)
        self.add_samples_flat(ids, off)

    def add_samples_tensors(self, ids, off):
        """Device form (bpe_add_sample_batch_device): ids a torch int32 tensor and off a torch int64
        tensor on the context's device."""
        import torch
        if ids.dtype != torch.int32 or off.dtype != torch.int64:
            raise BpeError('add_samples_tensors takes int32 ids and int64 offsets', ERR_ARG)
        if not (ids.is_cuda and off.is_cuda and ids.device == off.device):
            raise BpeError('add_samples_tensors takes tensors on the context\'s device', ERR_ARG)
        ids, off = ids.contiguous(), off.contiguous()
        torch.cuda.synchronize(ids.device)   # (the context runs on a stream of its own)
        _check(lib().bpe_add_sample_batch_device(self._ctx, ids.data_ptr() if ids.numel() else None,
                                                 off.data_ptr(), off.numel() - 1),
               'bpe_add_sample_batch_device')

    def restore_text_flat(self, enc, units, off):
        """Flat form (bpe_restore_text_batch): texts units[off[k]:off[k+1]] (UTF-16 units) are encoded
        by `enc` (an Encoder on the context's device: its chars, merges and long-text mode) and
        appended, each one sample.  The batch is atomic: on any error no text has been added."""
        units = np.ascontiguousarray(units, dtype=np.uint16).ravel()
        off = np.ascontiguousarray(off, dtype=np.int64)
        src = units if units.size else np.zeros(1, np.uint16)
        _check(lib().bpe_restore_text_batch(self._ctx, enc._enc if enc is not None else None, src.ctypes.data,
                                            off.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)), len(off) - 1),
               'bpe_restore_text_batch')

    def restore_text(self, enc, texts):
        """texts: a list of str (encoded with surrogatepass: lone surrogates survive)."""
        parts = [_units(t) for t in texts]
        off = np.zeros(len(parts) + 1, dtype=np.int64)
        np.cumsum([len(x) for x in parts], out=off[1:])
        units = np.concatenate(parts).astype(np.uint16) if parts and off[-1] else np.zeros(0, np.uint16)
        self.restore_text_flat(enc, units, off)

    def restore_text_tensors(self, enc, units, off):
        """Device form (bpe_restore_text_batch_device): units a torch int16 or uint16 tensor and off a
        torch int64 tensor on the context's device; no id comes to the host."""
        import torch
        if units.dtype not in (torch.int16, getattr(torch, 'uint16', torch.int16)) or off.dtype != torch.int64:
            raise BpeError('restore_text_tensors takes int16 or uint16 units and int64 offsets', ERR_ARG)
        if not (units.is_cuda and off.is_cuda and units.device == off.device):
            raise BpeError('restore_text_tensors takes tensors on the context\'s device', ERR_ARG)
        units, off = units.contiguous(), off.contiguous()
        torch.cuda.synchronize(units.device)   # (the context and the encoder run on streams of their own)
        _check(lib().bpe_restore_text_batch_device(self._ctx, enc._enc if enc is not None else None,
                                                   units.data_ptr() if units.numel() else None,
                                                   off.data_ptr(), off.numel() - 1),
               'bpe_restore_text_batch_device')

    # text as UTF-8 (include/bpe.h "text as UTF-8"): bytes in, transcoded on the device -----------------
    def add_utf8_batch(self, texts, off=None, new_cap=1024):
        """add_text for UTF-8: texts a list of bytes, or the flat form (uint8 array, int64 offsets).
        Each text decodes as bytes.decode('utf-8', 'replace') does -> (new_chars, hist)."""
        data, off = _utf8_flat(texts, off)
        src = data if data.size else np.zeros(1, np.uint8)
        return self._add_text(lib().bpe_add_utf8_batch, 'bpe_add_utf8_batch', src.ctypes.data,
                              off.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)), len(off) - 1, new_cap)

    def add_utf8_tensors(self, data, off, new_cap=1024):
        """Device form (bpe_add_utf8_batch_device): data a torch uint8 tensor (any byte offset) and
        off a torch int64 tensor on the context's device -> (new_chars, hist) as numpy arrays."""
        data, off = _utf8_tensors(data, off, 'add_utf8_tensors')
        return self._add_text(lib().bpe_add_utf8_batch_device, 'bpe_add_utf8_batch_device',
                              data.data_ptr() if data.numel() else None, off.data_ptr(), off.numel() - 1, new_cap)

    def restore_utf8_batch(self, enc, texts, off=None):
        """restore_text for UTF-8: texts a list of bytes, or the flat form (uint8 array, int64 offsets)."""
        data, off = _utf8_flat(texts, off)
        src = data if data.size else np.zeros(1, np.uint8)
        _check(lib().bpe_restore_utf8_batch(self._ctx, enc._enc if enc is not None else None, src.ctypes.data,
                                            off.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)), len(off) - 1),
               'bpe_restore_utf8_batch')

    def restore_utf8_tensors(self, enc, data, off):
        """Device form (bpe_restore_utf8_batch_device): torch uint8 bytes and int64 offsets on the
        context's device; neither a unit nor an id comes to the host."""
        data, off = _utf8_tensors(data, off, 'restore_utf8_tensors')
        _check(lib().bpe_restore_utf8_batch_device(self._ctx, enc._enc if enc is not None else None,
                                                   data.data_ptr() if data.numel() else None,
                                                   off.data_ptr(), off.numel() - 1),
               'bpe_restore_utf8_batch_device')

    def utf8_stats(self):
        s = Utf8Stats()
        _check(lib().bpe_get_utf8_stats(self._ctx, ctypes.byref(s)), 'bpe_get_utf8_stats')
        return s.as_dict()

    def reset_utf8_stats(self):
        _check(lib().bpe_reset_utf8_stats(self._ctx), 'bpe_reset_utf8_stats')

    # lines as samples (include/bpe.h "lines as samples"): the corpus helpers on the device ------------
    def _add_lines(self, name, mode, ptr, off_ptr, n, new_cap):
        mode, fn = lines_mode(mode), getattr(lib(), name)
        return self._add_text(lambda ctx, *rest: fn(ctx, mode, *rest), name, ptr, off_ptr, n, new_cap)

    def add_lines_flat(self, units, off, mode='trim', new_cap=1024):
        """Flat form (bpe_add_lines_batch): texts units[off[k]:off[k+1]] (UTF-16 units) are split into
        samples by the helper `mode` names ('trim': linesToCorpus, 'keep': linesTrimmedToCorpus,
        'file': fileContentToCorpus) and ingested as add_text ingests them -> (new_chars, hist)."""
        mode = lines_mode(mode)
        units = np.ascontiguousarray(units, dtype=np.uint16).ravel()
        off = np.ascontiguousarray(off, dtype=np.int64)
        src = units if units.size else np.zeros(1, np.uint16)
        return self._add_lines('bpe_add_lines_batch', mode, src.ctypes.data,
                               off.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)), len(off) - 1, new_cap)

    def add_lines(self, texts, mode='trim', new_cap=1024):
        """texts: a list of str (lone surrogates survive), each split into samples -> (new_chars, hist)."""
        units, off = _units_flat(texts)
        return self.add_lines_flat(units, off, mode, new_cap)

    def add_lines_tensors(self, units, off, mode='trim', new_cap=1024):
        """Device form (bpe_add_lines_batch_device): units a torch int16 or uint16 tensor and off a
        torch int64 tensor on the context's device -> (new_chars, hist) as numpy arrays."""
        mode = lines_mode(mode)
        units, off = _units_tensors(units, off, 'add_lines_tensors')
        return self._add_lines('bpe_add_lines_batch_device', mode, units.data_ptr() if units.numel() else None,
                               off.data_ptr(), off.numel() - 1, new_cap)

    def add_lines_utf8(self, texts, off=None, mode='trim', new_cap=1024):
        """add_lines for UTF-8: texts a list of bytes (files), or the flat form (uint8 array, int64
        offsets); transcoded and split on the device -> (new_chars, hist)."""
        mode = lines_mode(mode)
        data, off = _utf8_flat(texts, off)
        src = data if data.size else np.zeros(1, np.uint8)
        return self._add_lines('bpe_add_lines_utf8_batch', mode, src.ctypes.data,
                               off.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)), len(off) - 1, new_cap)

    def add_lines_utf8_tensors(self, data, off, mode='trim', new_cap=1024):
        """Device form (bpe_add_lines_utf8_batch_device): torch uint8 bytes and int64 offsets on the
        context's device -> (new_chars, hist) as numpy arrays."""
        mode = lines_mode(mode)
        data, off = _utf8_tensors(data, off, 'add_lines_utf8_tensors')
        return self._add_lines('bpe_add_lines_utf8_batch_device', mode, data.data_ptr() if data.numel() else None,
                               off.data_ptr(), off.numel() - 1, new_cap)

    def _restore_lines(self, name, enc, mode, ptr, off_ptr, n):
        _check(getattr(lib(), name)(self._ctx, enc._enc if enc is not None else None, mode, ptr, off_ptr, n), name)

    def restore_lines_flat(self, enc, units, off, mode='trim'):
        """Flat form (bpe_restore_lines_batch): the texts' samples are encoded by `enc` and appended,
        as restore_text appends them.  The batch is atomic."""
        mode = lines_mode(mode)
        units = np.ascontiguousarray(units, dtype=np.uint16).ravel()
        off = np.ascontiguousarray(off, dtype=np.int64)
        src = units if units.size else np.zeros(1, np.uint16)
        self._restore_lines('bpe_restore_lines_batch', enc, mode, src.ctypes.data,
                            off.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)), len(off) - 1)

    def restore_lines(self, enc, texts, mode='trim'):
        """texts: a list of str, each split into samples and restored."""
        self.restore_lines_flat(enc, *_units_flat(texts), mode)

    def restore_lines_tensors(self, enc, units, off, mode='trim'):
        """Device form (bpe_restore_lines_batch_device)."""
        mode = lines_mode(mode)
        units, off = _units_tensors(units, off, 'restore_lines_tensors')
        self._restore_lines('bpe_restore_lines_batch_device', enc, mode, units.data_ptr() if units.numel() else None,
                            off.data_ptr(), off.numel() - 1)

    def restore_lines_utf8(self, enc, texts, off=None, mode='trim'):
        """restore_lines for UTF-8: texts a list of bytes, or the flat form (uint8 array, int64 offsets)."""
        mode = lines_mode(mode)
        data, off = _utf8_flat(texts, off)
        src = data if data.size else np.zeros(1, np.uint8)
        self._restore_lines('bpe_restore_lines_utf8_batch', enc, mode, src.ctypes.data,
                            off.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)), len(off) - 1)

    def restore_lines_utf8_tensors(self, enc, data, off, mode='trim'):
        """Device form (bpe_restore_lines_utf8_batch_device)."""
        mode = lines_mode(mode)
        data, off = _utf8_tensors(data, off, 'restore_lines_utf8_tensors')
        self._restore_lines('bpe_restore_lines_utf8_batch_device', enc, mode, data.data_ptr() if data.numel() else None,
                            off.data_ptr(), off.numel() - 1)

    def lines_stats(self):
        s = LinesStats()
        _check(lib().bpe_get_lines_stats(self._ctx, ctypes.byref(s)), 'bpe_get_lines_stats')
        return s.as_dict()

    def reset_lines_stats(self):
        _check(lib().bpe_reset_lines_stats(self._ctx), 'bpe_reset_lines_stats')

    def token_counts(self):
        """Occurrences of every token id in the corpus (int64; the engine's own exact counts)."""
        out = np.zeros(MAX_VOCAB, np.int64)
        _check(lib().bpe_token_counts(self._ctx, out.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)), MAX_VOCAB),
               'bpe_token_counts')
        return out[:self.num_tokens()].copy()

    def append_stats(self):
        s = AppendStats()
        _check(lib().bpe_get_append_stats(self._ctx, ctypes.byref(s)), 'bpe_get_append_stats')
        return s.as_dict()

    def reset_append_stats(self):
        _check(lib().bpe_reset_append_stats(self._ctx), 'bpe_reset_append_stats')

    # corpus out (bpe_export_*, include/bpe.h) ---------------------------------------------------------
    _EXPORT_KINDS = {'ids': EXPORT_IDS, 'vectors': EXPORT_VECTORS, 'code': EXPORT_CODE, 'codes': EXPORT_CODE,
                     EXPORT_IDS: EXPORT_IDS, EXPORT_VECTORS: EXPORT_VECTORS, EXPORT_CODE: EXPORT_CODE}

    def _export_args(self, idx, kind, to_vector_index):
        """(kind, idx array or None, its pointer, n, index array or None, its pointer, its length)."""
        i32p, i64p = ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_int64)
        kind = self._EXPORT_KINDS[kind]
        if idx is None:
            idx_a, idx_p, n = None, None, self.corpus_size()[0]
        else:
            idx_a = np.ascontiguousarray(idx, np.int64).ravel()
            n = idx_a.size
            idx_p = (idx_a if n else np.zeros(1, np.int64)).ctypes.data_as(i64p)
        if to_vector_index is None:
            tvi_a, tvi_p, n_index = None, None, 0
        else:
            tvi_a = _i32(to_vector_index).ravel()
            n_index = tvi_a.size
            tvi_a = tvi_a if n_index else np.zeros(1, np.int32)
            tvi_p = tvi_a.ctypes.data_as(i32p)
        return kind, idx_a, idx_p, n, tvi_a, tvi_p, n_index

    def export_samples(self, idx=None, kind='ids', to_vector_index=None):
        """Samples out of the corpus (bpe_export_samples): idx a list of sample indices (any order,
        repeats allowed), None for every sample in corpus order; kind 'ids' (int32 token ids),
        'vectors' (int32 to_vector_index[id], encodeToVector of the sample) or 'code' (uint16 units
        id + 1, the sample's corpus_in_code string).  Returns (values, offsets int64) as numpy
        arrays.  A list of samples takes the sizing call first, then the real one."""
        kind, idx_a, idx_p, n, tvi_a, tvi_p, n_index = self._export_args(idx, kind, to_vector_index)
        i64p = ctypes.POINTER(ctypes.c_int64)
        dtype = np.uint16 if kind == EXPORT_CODE else np.int32
        off = np.zeros(n + 1, np.int64)
        if idx is None:   # (every sample: one value per live token, no sizing call)
            off[n] = self.corpus_size()[1]
        else:
            rc = lib().bpe_export_samples(self._ctx, kind, idx_p, n, tvi_p, n_index, None, 0,
                                          off.ctypes.data_as(i64p))
            if rc == BPE_OK:   # (nothing to write)
                return np.zeros(0, dtype), off
            if rc != ERR_ARG or off[n] <= 0:
                _check(rc, 'bpe_export_samples')
        vals = np.empty(max(int(off[n]), 1), dtype)[:int(off[n])]
        _check(lib().bpe_export_samples(self._ctx, kind, idx_p, n, tvi_p, n_index, vals.ctypes.data, vals.size,
                                        off.ctypes.data_as(i64p)), 'bpe_export_samples')
        return vals, off

    def export_samples_tensors(self, idx=None, kind='ids', to_vector_index=None, out=None):
        """Device form (bpe_export_samples_device): (values, offsets) as torch tensors on the context's
        device, int32 values (int16 for 'code') and int64 offsets; no value touches the host.  out: a
        tensor of that dtype on the device to write the values into (any element offset), else one
        is made after the sizing call."""
        import torch
        kind, idx_a, idx_p, n, tvi_a, tvi_p, n_index = self._export_args(idx, kind, to_vector_index)
        dev = torch.device('cuda', self.device)
        dtype = torch.int16 if kind == EXPORT_CODE else torch.int32
        off = torch.zeros(n + 1, dtype=torch.int64, device=dev)
        need = ctypes.c_int64()
        if out is None and idx is None:   # (every sample: one value per live token, no sizing call)
            out = torch.empty(self.corpus_size()[1], dtype=dtype, device=dev)
        if out is None:
            torch.cuda.synchronize(dev)   # (the context runs on a stream of its own)
            rc = lib().bpe_export_samples_device(self._ctx, kind, idx_p, n, tvi_p, n_index, None, 0, off.data_ptr(),
                                                 ctypes.byref(need))
            if rc == BPE_OK:
                return torch.zeros(0, dtype=dtype, device=dev), off
            if rc != ERR_ARG or need.value <= 0:
                _check(rc, 'bpe_export_samples_device')
            out = torch.empty(need.value, dtype=dtype, device=dev)
        elif out.dtype != dtype or not out.is_cuda or out.device.index != self.device or not out.is_contiguous():
            raise BpeError('export_samples_tensors takes a contiguous %s tensor on the context\'s device' % dtype,
                           ERR_ARG)
        torch.cuda.synchronize(dev)
        _check(lib().bpe_export_samples_device(self._ctx, kind, idx_p, n, tvi_p, n_index,
                                               out.data_ptr() if out.numel() else None, out.numel(),
                                               off.data_ptr(), ctypes.byref(need)), 'bpe_export_samples_device')
        return out[:need.value], off

    def export_text_flat(self, dec, idx=None):
        """Samples out as UTF-16 text through `dec` (a Decoder on the context's device;
        bpe_export_text_batch): (units uint16, offsets int64).  The sizing call, then the real one."""
        _, idx_a, idx_p, n, _, _, _ = self._export_args(idx, 'ids', None)
        i64p = ctypes.POINTER(ctypes.c_int64)
        d = dec._dec if dec is not None else None
        off = np.zeros(n + 1, np.int64)
        rc = lib().bpe_export_text_batch(self._ctx, d, idx_p, n, None, 0, off.ctypes.data_as(i64p))
        if rc == BPE_OK:
            return np.zeros(0, np.uint16), off
        if rc != ERR_ARG or off[n] <= 0:
            _check(rc, 'bpe_export_text_batch')
        units = np.empty(int(off[n]), np.uint16)
        _check(lib().bpe_export_text_batch(self._ctx, d, idx_p, n, units.ctypes.data, units.size,
                                           off.ctypes.data_as(i64p)), 'bpe_export_text_batch')
        return units, off

    def export_text(self, dec, idx=None):
        """The samples' texts as a list of str (lone surrogates kept)."""
        units, oo = self.export_text_flat(dec, idx)
        raw = units.astype('<u2', copy=False).tobytes()
        return [raw[2 * oo[k]:2 * oo[k + 1]].decode('utf-16-le', 'surrogatepass') for k in range(len(oo) - 1)]

    def export_text_tensors(self, dec, idx=None):
        """Device form (bpe_export_text_batch_device): (int16 tensor of the units, int64 offsets
        tensor) on the context's device; no id and no unit touches the host."""
        import torch
        _, idx_a, idx_p, n, _, _, _ = self._export_args(idx, 'ids', None)
        dev = torch.device('cuda', self.device)
        d = dec._dec if dec is not None else None
        off = torch.zeros(n + 1, dtype=torch.int64, device=dev)
        need = ctypes.c_int64()
        torch.cuda.synchronize(dev)
        rc = lib().bpe_export_text_batch_device(self._ctx, d, idx_p, n, None, 0, off.data_ptr(), ctypes.byref(need))
        if rc == BPE_OK:
            return torch.zeros(0, dtype=torch.int16, device=dev), off
        if rc != ERR_ARG or need.value <= 0:
            _check(rc, 'bpe_export_text_batch_device')
        units = torch.empty(need.value, dtype=torch.int16, device=dev)
        torch.cuda.synchronize(dev)
        _check(lib().bpe_export_text_batch_device(self._ctx, d, idx_p, n, units.data_ptr(), units.numel(),
                                                  off.data_ptr(), ctypes.byref(need)), 'bpe_export_text_batch_device')
        return units, off

    def export_utf8_flat(self, dec, idx=None):
        """Samples out as UTF-8 through `dec` (bpe_export_utf8_batch): (bytes uint8, offsets int64),
        encoded as Node's Buffer.from(text) encodes them.  The sizing call, then the real one."""
        _, idx_a, idx_p, n, _, _, _ = self._export_args(idx, 'ids', None)
        i64p = ctypes.POINTER(ctypes.c_int64)
        d = dec._dec if dec is not None else None
        off = np.zeros(n + 1, np.int64)
        rc = lib().bpe_export_utf8_batch(self._ctx, d, idx_p, n, None, 0, off.ctypes.data_as(i64p))
        if rc == BPE_OK:
            return np.zeros(0, np.uint8), off
        if rc != ERR_ARG or off[n] <= 0:
            _check(rc, 'bpe_export_utf8_batch')
        out = np.empty(int(off[n]), np.uint8)
        _check(lib().bpe_export_utf8_batch(self._ctx, d, idx_p, n, out.ctypes.data, out.size,
                                           off.ctypes.data_as(i64p)), 'bpe_export_utf8_batch')
        return out, off

    def export_utf8(self, dec, idx=None):
        """The samples' texts as a list of bytes."""
        out, oo = self.export_utf8_flat(dec, idx)
        raw = out.tobytes()
        return [raw[oo[k]:oo[k + 1]] for k in range(len(oo) - 1)]

    def export_utf8_tensors(self, dec, idx=None):
        """Device form (bpe_export_utf8_batch_device): (uint8 tensor of the bytes, int64 offsets
        tensor) on the context's device; no id, unit or byte touches the host."""
        import torch
        _, idx_a, idx_p, n, _, _, _ = self._export_args(idx, 'ids', None)
        dev = torch.device('cuda', self.device)
        d = dec._dec if dec is not None else None
        off = torch.zeros(n + 1, dtype=torch.int64, device=dev)
        need = ctypes.c_int64()
        torch.cuda.synchronize(dev)
        rc = lib().bpe_export_utf8_batch_device(self._ctx, d, idx_p, n, None, 0, off.data_ptr(), ctypes.byref(need))
        if rc == BPE_OK:
            return torch.zeros(0, dtype=torch.uint8, device=dev), off
        if rc != ERR_ARG or need.value <= 0:
            _check(rc, 'bpe_export_utf8_batch_device')
        out = torch.empty(need.value, dtype=torch.uint8, device=dev)
        torch.cuda.synchronize(dev)
        _check(lib().bpe_export_utf8_batch_device(self._ctx, d, idx_p, n, out.data_ptr(), out.numel(),
                                                  off.data_ptr(), ctypes.byref(need)), 'bpe_export_utf8_batch_device')
        return out, off

    def export_stats(self):
        s = ExportStats()
        _check(lib().bpe_get_export_stats(self._ctx, ctypes.byref(s)), 'bpe_get_export_stats')
        return s.as_dict()

    def reset_export_stats(self):
        _check(lib().bpe_reset_export_stats(self._ctx), 'bpe_reset_export_stats')

    # skip-gram pairs of corpus samples (include/bpe.h "skip-gram pairs") -----------------------------
    def export_skipgram(self, idx=None, window=2, kind='vectors', to_vector_index=None):
        """Corpus samples expanded into the (target, context) pairs of example/skip-gram.ts's loop on
        the device (bpe_export_skipgram): idx, kind ('vectors' or 'ids') and to_vector_index as in
        export_samples -> (targets int32, contexts int32, pair_off int64) as numpy arrays.  The sizing
        call, then the real one."""
        kind, idx_a, idx_p, n, tvi_a, tvi_p, n_index = self._export_args(idx, kind, to_vector_index)
        return _skipgram_host('bpe_export_skipgram', lambda t, c, cap, po: lib().bpe_export_skipgram(
            self._ctx, kind, idx_p, n, tvi_p, n_index, int(window), t, c, cap, po), n)

    def export_skipgram_tensors(self, idx=None, window=2, kind='vectors', to_vector_index=None, out=None):
        """Device form (bpe_export_skipgram_device): (targets, contexts, pair_off) as torch tensors on
        the context's device, two int32 planes and int64 offsets; no value touches the host.  out: a
        pair of contiguous int32 tensors on the device to write the planes into, else a sizing call
        runs first."""
        kind, idx_a, idx_p, n, tvi_a, tvi_p, n_index = self._export_args(idx, kind, to_vector_index)
        return _skipgram_device('bpe_export_skipgram_device', lambda t, c, cap, po, need: lib().bpe_export_skipgram_device(
            self._ctx, kind, idx_p, n, tvi_p, n_index, int(window), t, c, cap, po, need), n, self.device, out)

    def skipgram_stats(self):
        s = SkipgramStats()
        _check(lib().bpe_get_skipgram_stats(self._ctx, ctypes.byref(s)), 'bpe_get_skipgram_stats')
        return s.as_dict()

    def reset_skipgram_stats(self):
        _check(lib().bpe_reset_skipgram_stats(self._ctx), 'bpe_reset_skipgram_stats')

    def clear_corpus(self):
        _check(lib().bpe_clear_corpus(self._ctx), 'bpe_clear_corpus')

    def corpus_size(self):
        s, t = ctypes.c_int64(), ctypes.c_int64()
        _check(lib().bpe_corpus_size(self._ctx, ctypes.byref(s), ctypes.byref(t)), 'bpe_corpus_size')
        return s.value, t.value

    def read_corpus(self):
        """Returns (flat ids int32, sample offsets int64)."""
        ns, nt = self.corpus_size()
        ids = np.zeros(max(nt, 1), np.int32)
        off = np.zeros(ns + 1, np.int64)
        _check(lib().bpe_read_corpus(self._ctx, ids.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)),
                                     ids.size, off.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)),
                                     off.size), 'bpe_read_corpus')
        return ids[:nt], off

    def sample_lengths(self):
        """Live tokens per sample (int64), from the device-side sample index."""
        ns, _ = self.corpus_size()
        lens = np.zeros(max(ns, 1), np.int64)
        _check(lib().bpe_sample_lengths(self._ctx, lens.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)),
                                        lens.size), 'bpe_sample_lengths')
        return lens[:ns]

    def read_samples(self, idx):
        """The listed samples' ids: (flat ids int32, offsets int64), in the order of idx."""
        idx = np.ascontiguousarray(idx, np.int64)
        lens = self.sample_lengths()
        need = int(lens[idx].sum()) if idx.size else 0
        ids = np.zeros(max(need, 1), np.int32)
        off = np.zeros(idx.size + 1, np.int64)
        _check(lib().bpe_read_samples(self._ctx, idx.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)),
                                      idx.size, ids.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)),
                                      ids.size, off.ctypes.data_as(ctypes.POINTER(ctypes.c_int64))),
               'bpe_read_samples')
        return ids[:need], off

    def samples(self):
        ids, off = self.read_corpus()
        return [ids[off[i]:off[i + 1]].tolist() for i in range(len(off) - 1)]

    # hot path ----------------------------------------------------------------------------------
    def find_next_merge(self, max_length=0, min_weight=0):
        a, b, w = ctypes.c_int32(), ctypes.c_int32(), ctypes.c_int64()
        rc = _check(lib().bpe_find_next_merge(self._ctx, int(max_length or 0), int(min_weight or 0),
                                              ctypes.byref(a), ctypes.byref(b), ctypes.byref(w)),
                    'bpe_find_next_merge')
        return None if rc == BPE_NO_MERGE else (a.value, b.value, w.value)

    def apply_merge(self, a, b, c, sync=True):
        """applyMerge's corpus rewrite.  With sync=False the replacement count stays on the device
        (settled at the next engine call; no host round trip) and None is returned."""
        if not sync:
            _check(lib().bpe_apply_merge(self._ctx, a, b, c, None), 'bpe_apply_merge')
            return None
        r = ctypes.c_int64()
        _check(lib().bpe_apply_merge(self._ctx, a, b, c, ctypes.byref(r)), 'bpe_apply_merge')
        return r.value

    def apply_merges(self, merges, count_after=True):
        """restoreMerge replay / batch encoding (bpe_apply_merges): applies the (a, b, c) triples
        in order without counting pairs; returns the replacement counts."""
        abc = np.ascontiguousarray(np.asarray(merges, np.int32).reshape(-1, 3))
        rep = np.zeros(len(abc), np.int64)
        _check(lib().bpe_apply_merges(self._ctx, abc.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)),
                                      len(abc), rep.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)),
                                      1 if count_after else 0), 'bpe_apply_merges')
        return rep.tolist()

    def merge_until(self, max_length=0, min_weight=0, max_iterations=0, cap=1 << 16):
        out = np.zeros(3 * cap, np.int64)
        n = ctypes.c_int64()
        _check(lib().bpe_merge_until(self._ctx, int(max_length or 0), int(min_weight or 0),
                                     int(max_iterations or 0),
                                     out.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)), cap,
                                     ctypes.byref(n)), 'bpe_merge_until')
        k = min(n.value, cap)
        return [tuple(int(v) for v in out[3 * i:3 * i + 3]) for i in range(k)]

    # measurement -------------------------------------------------------------------------------
    def stats_enable(self, on=True):
        _check(lib().bpe_stats_enable(self._ctx, 1 if on else 0), 'bpe_stats_enable')

    def stats(self):
        s = Stats()
        _check(lib().bpe_get_stats(self._ctx, ctypes.byref(s)), 'bpe_get_stats')
        return s.as_dict()

    # sharded corpus (device pointers, e.g. torch tensors' data_ptr()) ------------------------------
    def export_counts(self, table_ptr):
        """Copies this shard's [TABLE_BINS] u64 table (hot bins + cold sketch) to device memory."""
        _check(lib().bpe_export_counts(self._ctx, table_ptr), 'bpe_export_counts')

    def heavy_counts(self, table_ptr, keys_ptr, counts_ptr, cap, max_length=0):
        """Exact shard counts of the cold pairs whose GLOBAL sketch bucket could still win.
        Returns the entry count (> cap means nothing was written: grow and retry; -1 means no
        bucket qualified, which every rank decides alike)."""
        n = ctypes.c_int64()
        rc = lib().bpe_heavy_counts(self._ctx, table_ptr, int(max_length or 0), keys_ptr,
                                    counts_ptr, cap, ctypes.byref(n))
        if rc < 0 and n.value <= cap:
            _check(rc, 'bpe_heavy_counts')
        return n.value

    def select_counts(self, table_ptr, keys_ptr, counts_ptr, n_cold, max_length=0, min_weight=0,
                      cap=4096):
        """Selection over global tables: None, or (W, [(a, b), ...] candidates sorted)."""
        cand = np.zeros(2 * cap, np.int32)
        n, w = ctypes.c_int64(), ctypes.c_int64()
        rc = _check(lib().bpe_select_counts(self._ctx, table_ptr, keys_ptr, counts_ptr, n_cold,
                                            int(max_length or 0), int(min_weight or 0),
                                            cand.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)),
                                            cap, ctypes.byref(n), ctypes.byref(w)),
                    'bpe_select_counts')
        if rc == BPE_NO_MERGE:
            return None
        if n.value > cap:
            raise BpeError('more than %d tied candidates' % cap)
        return w.value, [(int(cand[2 * i]), int(cand[2 * i + 1])) for i in range(n.value)]

    def tie_positions(self, cands):
        """Shard-local last counted occurrence (+1, 0 = none) of each (a, b) candidate (R3)."""
        c = np.ascontiguousarray(np.asarray(cands, np.int32).reshape(-1))
        last = np.zeros(len(cands), np.uint64)
        _check(lib().bpe_tie_positions(self._ctx, c.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)),
                                       len(cands), last.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64))),
               'bpe_tie_positions')
        return last

    # device-resident loop on one rank (bpe.h: bpe_rank_loop_*); the caller all-reduces `table`
    # and `tie` in order on stream() between the calls
    def stream(self):
        st = ctypes.c_void_p()
        _check(lib().bpe_get_stream(self._ctx, ctypes.byref(st)), 'bpe_get_stream')
        return st.value or 0

    def rank_loop_begin(self, max_length, min_weight, xchg_ptr, tie_ptr, rank, world):
        """Returns the number of exchange words to all-reduce per iteration of this batch."""
        nw = ctypes.c_int64()
        _check(lib().bpe_rank_loop_begin(self._ctx, int(max_length or 0), int(min_weight or 0),
                                         xchg_ptr, tie_ptr, rank, world, ctypes.byref(nw)),
               'bpe_rank_loop_begin')
        return nw.value

    def rank_loop_select(self):
        _check(lib().bpe_rank_loop_select(self._ctx), 'bpe_rank_loop_select')

    def rank_loop_decide(self):
        _check(lib().bpe_rank_loop_decide(self._ctx), 'bpe_rank_loop_decide')

    def rank_loop_count(self):
        _check(lib().bpe_rank_loop_count(self._ctx), 'bpe_rank_loop_count')

    def rank_loop_end(self):
        """Syncs; returns ([(a, b, W)] merged in this batch, [this shard's replacement count of
        each], status) with status 0 = run on, 1 = no pair qualifies, 2 = the next iteration needs
        the host protocol."""
        out = np.zeros(4 * LOOP_BATCH, np.int64)
        n, st = ctypes.c_int64(), ctypes.c_int()
        _check(lib().bpe_rank_loop_end(self._ctx, out.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)),
                                       LOOP_BATCH, ctypes.byref(n), ctypes.byref(st)),
               'bpe_rank_loop_end')
        k = n.value
        return ([tuple(int(v) for v in out[4 * i:4 * i + 3]) for i in range(k)],
                [int(out[4 * i + 3]) for i in range(k)], st.value)

    def rccl_init(self, unique_id, rank, world):
        """This context's RCCL communicator (bpe_rank_rccl_init); unique_id: 128 bytes made by
        rccl_unique_id() on rank 0 and broadcast."""
        buf = ctypes.create_string_buffer(bytes(unique_id), 128)
        _check(lib().bpe_rank_rccl_init(self._ctx, buf, int(rank), int(world)), 'bpe_rank_rccl_init')

    def rank_loop_rccl(self, xchg_ptr, xchg_words, tie_ptr, iterations):
        """`iterations` rank-loop iterations with their all-reduces from C++ (bpe_rank_loop_rccl)."""
        _check(lib().bpe_rank_loop_rccl(self._ctx, xchg_ptr, int(xchg_words), tie_ptr, int(iterations)),
               'bpe_rank_loop_rccl')

    def cold_counts(self, keys_ptr, counts_ptr, cap):
        """This shard's exact count of every cold pair (one pass, kept for a second call): the
        entry count (> cap: nothing written, call again with room)."""
        n = ctypes.c_int64()
        _check(lib().bpe_cold_counts(self._ctx, keys_ptr, counts_ptr, cap, ctypes.byref(n)),
               'bpe_cold_counts')
        return n.value

    def set_global_counts(self, table_ptr, keys_ptr, counts_ptr, n):
        """The maintained state of a sharded corpus: the global table and every shard's cold
        lists (device pointers, duplicates summed) become this rank's global tables."""
        _check(lib().bpe_set_global_counts(self._ctx, table_ptr, keys_ptr, counts_ptr, n),
               'bpe_set_global_counts')

    def recount(self):
        """One plain streaming count pass (K1 alone; measurement helper)."""
        _check(lib().bpe_recount(self._ctx), 'bpe_recount')

    def reset_stats(self):
        _check(lib().bpe_reset_stats(self._ctx), 'bpe_reset_stats')

    # the maintained tables, for checking (include/bpe_tools.h) -------------------------------------
    def is_maintained(self):
        """Whether the context holds the single-context maintained state (bpe_table_state)."""
        m = ctypes.c_int()
        _check(lib().bpe_table_state(self._ctx, ctypes.byref(m)), 'bpe_table_state')
        return bool(m.value)

    def maintained_tables(self, shard=None):
        """(hot, keys, counts): the HOT_BINS u64 hot bins (pair (a, b) at b * 256 + a) and the
        cold table's dense entries (key a << 16 | b as uint32, count as uint64; bpe_debug_tables:
        the sizing call, then the real one).  shard=k: the copy of the global tables that shard k
        of a multi-device context holds (bpe_debug_tables_shard)."""
        L = lib()
        hot = np.zeros(HOT_BINS, np.uint64)
        n = ctypes.c_int64()

        def call(keys, counts, cap):
            if shard is None:
                _check(L.bpe_debug_tables(self._ctx, hot.ctypes.data, keys, counts, cap, ctypes.byref(n)),
                       'bpe_debug_tables')
            else:
                _check(L.bpe_debug_tables_shard(self._ctx, int(shard), hot.ctypes.data, keys, counts, cap,
                                                ctypes.byref(n)), 'bpe_debug_tables_shard')

        call(None, None, 0)
        keys = np.zeros(max(n.value, 1), np.uint32)
        counts = np.zeros(max(n.value, 1), np.uint64)
        cap = n.value
        if cap:
            call(keys.ctypes.data, counts.ctypes.data, cap)
        k = min(n.value, cap)
        return hot, keys[:k], counts[:k]

    def global_state(self, shard=None):
        """(state, xchg) of bpe_debug_global: what this context (a single context used as one rank)
        or shard `shard` of a multi-device context holds of the streaming mode's sharded
        maintained state, as a dict of the GLOBAL_INFO words with 'held' and 'pending' as bools,
        and a copy of the exchange buffer it last began a batch with (uint64, XCHG_WORDS words
        while the state is held, else empty)."""
        L = lib()
        info = (ctypes.c_int64 * len(GLOBAL_INFO))()
        sh = -1 if shard is None else int(shard)
        _check(L.bpe_debug_global(self._ctx, sh, info, None, 0), 'bpe_debug_global')
        words = int(info[GLOBAL_INFO.index('xchg_words')])
        xchg = np.zeros(max(words, 1), np.uint64)
        if words:
            _check(L.bpe_debug_global(self._ctx, sh, info, xchg.ctypes.data, words), 'bpe_debug_global')
        state = {name: int(info[i]) for i, name in enumerate(GLOBAL_INFO)}
        state['held'], state['pending'] = bool(state['held']), bool(state['pending'])
        return state, xchg[:min(words, state['xchg_words'])]

    # the position index of the incremental mode, for checking (include/bpe_tools.h) ----------------
    def pix_view(self, shard=None):
        """The live position index copied out (bpe_debug_pix; shard=k: shard k of a multi-device
        context, bpe_debug_pix_shard): a dict of the PIX_INFO scalars and the PIX_ARRAYS numpy
        arrays, or None when the context holds no index."""
        L = lib()
        info = (ctypes.c_int64 * PIX_INFO_WORDS)()

        def call(arrays):
            if shard is None:
                _check(L.bpe_debug_pix(self._ctx, info, arrays), 'bpe_debug_pix')
            else:
                _check(L.bpe_debug_pix_shard(self._ctx, int(shard), info, arrays), 'bpe_debug_pix_shard')

        call(None)
        v = {name: int(info[i]) for i, name in enumerate(PIX_INFO)}
        if not v['present']:
            return None
        sizes = {'n': v['n'], 'cap': v['cap'], 'nblocks': v['nblocks'], 'nsuper': v['nsuper'],
                 'pool_top': v['pool_top'], 'n_dblocks': v['n_dblocks'], 'n_dsuper': v['n_dsuper']}
        ptrs = (ctypes.c_void_p * len(PIX_ARRAYS))()
        for i, (name, dt, size) in enumerate(PIX_ARRAYS):
            v[name] = np.zeros(max(sizes[size], 1), dt)
            ptrs[i] = v[name].ctypes.data
        call(ptrs)
        for name, _, size in PIX_ARRAYS:
            v[name] = v[name][:sizes[size]]
        return v

    def pix_hook(self, fn, batch=0):
        """fn(where) is called by merge_until in the incremental mode while its index is live
        (bpe_debug_pix_hook: where 0 before a batch, 1 after one), with `batch` iterations per
        batch (0: the default).  fn may call pix_view and must not raise: ctypes drops an
        exception raised in a callback, so a checker records its findings and the caller asserts
        on them afterwards.  fn=None removes the hook."""
        cb = PIX_HOOK((lambda user, where: fn(where)) if fn is not None else 0)
        _check(lib().bpe_debug_pix_hook(self._ctx, cb, None, int(batch)), 'bpe_debug_pix_hook')
        self._pix_hook = cb   # (kept alive while the library holds it)


class Encoder:
    """encodeToCode (core.ts:392-409) for batches of texts with a trained merge list, apart from
    any corpus (bpe_encoder_*, include/bpe.h): the merge list lives on the device as a rank table;
    texts up to ENCODE_LDS_TOKENS tokens are encoded by the merge-rank kernel (csrc/bpe_encode.hip), longer
    ones by apply-only replay passes, or (long_texts='split') as segments cut at boundaries no
    merge can cross.  long_texts=None keeps the library's choice (BPE_ENCODE_LONG in the
    environment, else 'replay').  No CPU fallback."""

    _LONG = {'replay': LONG_REPLAY, 'split': LONG_SPLIT}

    def __init__(self, device=0, merges=None, long_texts=None):
        p = ctypes.c_void_p()
        _check(lib().bpe_encoder_create(ctypes.byref(p), int(device)), 'bpe_encoder_create')
        self._enc = p
        self.device = int(device)
        if long_texts is not None:
            self.set_long_texts(long_texts)
        if merges is not None and len(merges):
            self.add_merges(merges)

    def close(self):
        if self._enc:
            lib().bpe_encoder_destroy(self._enc)
            self._enc = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def add_merges(self, merges):
        """Appends (a, b, c) triples in list order (merge_codes, core.ts:91,352)."""
        abc = _i32(np.asarray(merges, dtype=np.int32).reshape(-1))
        _check(lib().bpe_encoder_add_merges(self._enc, abc.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)),
                                            len(abc) // 3), 'bpe_encoder_add_merges')

    def clear(self):
        _check(lib().bpe_encoder_clear(self._enc), 'bpe_encoder_clear')

    def num_merges(self):
        n = ctypes.c_int64()
        _check(lib().bpe_encoder_num_merges(self._enc, ctypes.byref(n)), 'bpe_encoder_num_merges')
        return n.value

    def encode_flat(self, ids, off):
        """Flat form: texts ids[off[k]:off[k+1]] -> (ids_out, out_off) numpy arrays."""
        ids = _i32(ids)
        off = np.ascontiguousarray(off, dtype=np.int64)
        n = len(off) - 1
        total = int(off[-1] - off[0]) if n > 0 else 0
        out = np.zeros(max(total, 1), dtype=np.int32)
        out_off = np.zeros(max(n + 1, 1), dtype=np.int64)
        src = ids if ids.size else np.zeros(1, np.int32)
        i32p, i64p = ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_int64)
        _check(lib().bpe_encode_batch(self._enc, src.ctypes.data_as(i32p), off.ctypes.data_as(i64p),
                                      n, out.ctypes.data_as(i32p), out_off.ctypes.data_as(i64p)),
               'bpe_encode_batch')
        return out[:out_off[n] if n > 0 else 0], out_off

    def encode(self, texts):
        """texts: a list of id sequences -> list of encoded int32 arrays."""
        lens = [len(t) for t in texts]
        off = np.zeros(len(texts) + 1, dtype=np.int64)
        np.cumsum(lens, out=off[1:])
        ids = np.concatenate([np.asarray(t, dtype=np.int32) for t in texts]) if texts and off[-1] \
            else np.zeros(0, np.int32)
        out, oo = self.encode_flat(ids, off)
        return [out[oo[k]:oo[k + 1]].copy() for k in range(len(texts))]

    def stats(self):
        s = EncoderStats()
        _check(lib().bpe_encoder_get_stats(self._enc, ctypes.byref(s)), 'bpe_encoder_get_stats')
        return s.as_dict()

    def reset_stats(self):
        _check(lib().bpe_encoder_reset_stats(self._enc), 'bpe_encoder_reset_stats')

    def set_long_texts(self, mode):
        """'replay' or 'split' (or LONG_REPLAY / LONG_SPLIT): how texts of more than
        ENCODE_LDS_TOKENS tokens are encoded (bpe_encoder_set_long_texts)."""
        _check(lib().bpe_encoder_set_long_texts(self._enc, int(self._LONG.get(mode, mode))),
               'bpe_encoder_set_long_texts')

    def split_stats(self):
        s = SplitStats()
        _check(lib().bpe_encoder_get_split_stats(self._enc, ctypes.byref(s)), 'bpe_encoder_get_split_stats')
        return s.as_dict()

    def reset_split_stats(self):
        _check(lib().bpe_encoder_reset_split_stats(self._enc), 'bpe_encoder_reset_split_stats')

    # the text form: encodeToVector (core.ts:392-445) from UTF-16 units ---------------------------
    _KINDS = {'ids': ENCODE_IDS, 'tokens': ENCODE_IDS, 'vectors': ENCODE_VECTORS,
              ENCODE_IDS: ENCODE_IDS, ENCODE_VECTORS: ENCODE_VECTORS}

    def set_chars(self, mapping):
        """Replaces the char table (char_to_token): a dict of a str of one code point (a lone
        surrogate included), or an int code point, to a token id.  An empty dict drops it."""
        cps = np.asarray([ord(k) if isinstance(k, str) else int(k) for k in mapping], dtype=np.uint32)
        ids = _i32(list(mapping.values()))
        cbuf = cps if cps.size else np.zeros(1, np.uint32)
        ibuf = ids if ids.size else np.zeros(1, np.int32)
        _check(lib().bpe_encoder_set_chars(self._enc, cbuf.ctypes.data,
                                           ibuf.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), cps.size),
               'bpe_encoder_set_chars')

    def set_vector_index(self, to_vector_index):
        """to_vector_index of compactVectorIndex (core.ts:222-241): one entry per token id, -1
        for a hole; None drops the index."""
        if to_vector_index is None:
            _check(lib().bpe_encoder_set_vector_index(self._enc, None, 0), 'bpe_encoder_set_vector_index')
            return
        a = _i32(to_vector_index).ravel()
        buf = a if a.size else np.zeros(1, np.int32)
        _check(lib().bpe_encoder_set_vector_index(self._enc, buf.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)),
                                                  a.size), 'bpe_encoder_set_vector_index')

    def encode_text_flat(self, units, off, kind='vectors'):
        """Flat form: texts units[off[k]:off[k+1]] (UTF-16 units) -> (values int32, out_off int64)."""
        kind = self._KINDS[kind]
        units = np.ascontiguousarray(units, dtype=np.uint16).ravel()
        off = np.ascontiguousarray(off, dtype=np.int64)
        n = len(off) - 1
        total = max(int(off[-1] - off[0]), 0) if n > 0 else 0
        out = np.zeros(max(total, 1), dtype=np.int32)
        out_off = np.zeros(n + 1, dtype=np.int64)
        src = units if units.size else np.zeros(1, np.uint16)
        _check(lib().bpe_encode_text_batch(self._enc, kind, src.ctypes.data,
                                           off.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)), n,
                                           out.ctypes.data, out.size,
                                           out_off.ctypes.data_as(ctypes.POINTER(ctypes.c_int64))),
               'bpe_encode_text_batch')
        return out[:out_off[n]], out_off

    def encode_text(self, texts, kind='vectors'):
        """texts: a list of str (encoded with surrogatepass: lone surrogates survive) -> list of
        int32 arrays of vector indices (or token ids, kind='ids')."""
        parts = [_units(t) for t in texts]
        off = np.zeros(len(parts) + 1, dtype=np.int64)
        np.cumsum([len(x) for x in parts], out=off[1:])
        units = np.concatenate(parts).astype(np.uint16) if parts and off[-1] else np.zeros(0, np.uint16)
        out, oo = self.encode_text_flat(units, off, kind)
        return [out[oo[k]:oo[k + 1]].copy() for k in range(len(parts))]

    def encode_text_tensors(self, units, off, kind='vectors'):
        """Device form (bpe_encode_text_batch_device): units a torch int16 or uint16 tensor and off
        a torch int64 tensor on the encoder's device -> (int32 tensor of the values, int64 offsets
        tensor), both on that device."""
        import torch
        kind = self._KINDS[kind]
        if units.dtype not in (torch.int16, getattr(torch, 'uint16', torch.int16)) or off.dtype != torch.int64:
            raise BpeError('encode_text_tensors takes int16 or uint16 units and int64 offsets', ERR_ARG)
        if not (units.is_cuda and off.is_cuda and units.device.index == self.device
                and off.device.index == self.device):
            raise BpeError('encode_text_tensors takes tensors on the encoder\'s device', ERR_ARG)
        units, off = units.contiguous(), off.contiguous()
        n = off.numel() - 1
        vals = torch.empty(max(units.numel(), 1), dtype=torch.int32, device=units.device)
        out_off = torch.zeros(n + 1, dtype=torch.int64, device=units.device)
        torch.cuda.synchronize(units.device)   # (the encoder runs on a stream of its own)
        need = ctypes.c_int64()
        up = units.data_ptr() if units.numel() else None
        _check(lib().bpe_encode_text_batch_device(self._enc, kind, up, off.data_ptr(), n, vals.data_ptr(),
                                                  units.numel(), out_off.data_ptr(), ctypes.byref(need)),
               'bpe_encode_text_batch_device')
        return vals[:need.value], out_off

    def text_stats(self):
        s = TextStats()
        _check(lib().bpe_encoder_get_text_stats(self._enc, ctypes.byref(s)), 'bpe_encoder_get_text_stats')
        return s.as_dict()

    def reset_text_stats(self):
        _check(lib().bpe_encoder_reset_text_stats(self._enc), 'bpe_encoder_reset_text_stats')


    # text as UTF-8 (include/bpe.h "text as UTF-8"): bytes in, transcoded on the device -----------------
    def utf8_to_utf16(self, texts, off=None):
        """The transcode alone: texts a list of bytes, or the flat form (uint8 array, int64 offsets)
        -> (units uint16, out_off int64).  Each text decodes as bytes.decode('utf-8', 'replace')."""
        data, off = _utf8_flat(texts, off)
        n = len(off) - 1
        total = max(int(off[-1] - off[0]), 0) if n > 0 else 0
        units = np.zeros(max(total, 1), dtype=np.uint16)
        out_off = np.zeros(n + 1, dtype=np.int64)
        src = data if data.size else np.zeros(1, np.uint8)
        i64p = ctypes.POINTER(ctypes.c_int64)
        _check(lib().bpe_encoder_utf8_to_utf16(self._enc, src.ctypes.data, off.ctypes.data_as(i64p), n,
                                               units.ctypes.data, units.size, out_off.ctypes.data_as(i64p)),
               'bpe_encoder_utf8_to_utf16')
        return units[:out_off[n]], out_off

    def utf8_to_utf16_tensors(self, data, off):
        """Device form (bpe_encoder_utf8_to_utf16_device): data a torch uint8 tensor (any byte offset)
        and off a torch int64 tensor on the encoder's device -> (int16 tensor of the units, int64
        offsets tensor), both on that device."""
        import torch
        data, off = _utf8_tensors(data, off, 'utf8_to_utf16_tensors', self.device)
        n = off.numel() - 1
        units = torch.empty(max(data.numel(), 1), dtype=torch.int16, device=data.device)
        out_off = torch.zeros(n + 1, dtype=torch.int64, device=data.device)
        torch.cuda.synchronize(data.device)
        need = ctypes.c_int64()
        _check(lib().bpe_encoder_utf8_to_utf16_device(self._enc, data.data_ptr() if data.numel() else None,
                                                      off.data_ptr(), n, units.data_ptr(), units.numel(),
                                                      out_off.data_ptr(), ctypes.byref(need)),
               'bpe_encoder_utf8_to_utf16_device')
        return units[:need.value], out_off

    def encode_utf8(self, texts, off=None, kind='vectors'):
        """encode_text for UTF-8.  texts a list of bytes -> list of int32 arrays; the flat form
        (uint8 array, int64 offsets) -> (values int32, out_off int64)."""
        kind = self._KINDS[kind]
        flat = off is not None
        data, off = _utf8_flat(texts, off)
        n = len(off) - 1
        total = max(int(off[-1] - off[0]), 0) if n > 0 else 0
        out = np.zeros(max(total, 1), dtype=np.int32)
        out_off = np.zeros(n + 1, dtype=np.int64)
        src = data if data.size else np.zeros(1, np.uint8)
        i64p = ctypes.POINTER(ctypes.c_int64)
        _check(lib().bpe_encode_utf8_batch(self._enc, kind, src.ctypes.data, off.ctypes.data_as(i64p), n,
                                           out.ctypes.data, out.size, out_off.ctypes.data_as(i64p)),
               'bpe_encode_utf8_batch')
        if flat:
            return out[:out_off[n]], out_off
        return [out[out_off[k]:out_off[k + 1]].copy() for k in range(n)]

    def encode_utf8_tensors(self, data, off, kind='vectors'):
        """Device form (bpe_encode_utf8_batch_device): torch uint8 bytes and int64 offsets on the
        encoder's device -> (int32 tensor of the values, int64 offsets tensor), both on that device."""
        import torch
        kind = self._KINDS[kind]
        data, off = _utf8_tensors(data, off, 'encode_utf8_tensors', self.device)
        n = off.numel() - 1
        vals = torch.empty(max(data.numel(), 1), dtype=torch.int32, device=data.device)
        out_off = torch.zeros(n + 1, dtype=torch.int64, device=data.device)
        torch.cuda.synchronize(data.device)   # (the encoder runs on a stream of its own)
        need = ctypes.c_int64()
        _check(lib().bpe_encode_utf8_batch_device(self._enc, kind, data.data_ptr() if data.numel() else None,
                                                  off.data_ptr(), n, vals.data_ptr(), data.numel(),
                                                  out_off.data_ptr(), ctypes.byref(need)),
               'bpe_encode_utf8_batch_device')
        return vals[:need.value], out_off

    def utf8_stats(self):
        s = Utf8Stats()
        _check(lib().bpe_encoder_get_utf8_stats(self._enc, ctypes.byref(s)), 'bpe_encoder_get_utf8_stats')
        return s.as_dict()

    def reset_utf8_stats(self):
        _check(lib().bpe_encoder_reset_utf8_stats(self._enc), 'bpe_encoder_reset_utf8_stats')

    # lines as samples (include/bpe.h "lines as samples"): the corpus helpers on the device ------------
    def split_lines_flat(self, units, off, mode='trim'):
        """The split alone (bpe_encoder_split_lines): texts units[off[k]:off[k+1]] (UTF-16 units) ->
        (units uint16, out_off int64) of the samples the helper `mode` names makes of them ('trim':
        linesToCorpus, 'keep': linesTrimmedToCorpus, 'file': fileContentToCorpus)."""
        mode = lines_mode(mode)
        units = np.ascontiguousarray(units, dtype=np.uint16).ravel()
        off = np.ascontiguousarray(off, dtype=np.int64)
        n = len(off) - 1
        if n > 0 and (off[0] < 0 or np.any(np.diff(off) < 0)):
            raise BpeError('split_lines: text offsets must not decrease', ERR_ARG)
        total = int(off[-1] - off[0]) if n > 0 else 0
        out = np.zeros(max(3 * total + 2 * n, 1), dtype=np.uint16)
        out_off = np.zeros(total + n + 1, dtype=np.int64)
        src = units if units.size else np.zeros(1, np.uint16)
        i64p = ctypes.POINTER(ctypes.c_int64)
        ns = ctypes.c_int64()
        _check(lib().bpe_encoder_split_lines(self._enc, mode, src.ctypes.data, off.ctypes.data_as(i64p), n,
                                             out.ctypes.data, out.size, out_off.ctypes.data_as(i64p), out_off.size,
                                             ctypes.byref(ns)), 'bpe_encoder_split_lines')
        out_off = out_off[:ns.value + 1].copy()
        return out[:out_off[-1]].copy(), out_off

    def split_lines(self, texts, mode='trim'):
        """texts: a list of str (lone surrogates survive) -> the list of str texts.flatMap(helper) gives."""
        units, off = _units_flat(texts)
        out, oo = self.split_lines_flat(units, off, mode)
        return [units_to_str(out[oo[k]:oo[k + 1]]) for k in range(len(oo) - 1)]

    def split_lines_tensors(self, units, off, mode='trim', out=None, out_off=None):
        """Device form (bpe_encoder_split_lines_device): units a torch int16 or uint16 tensor and off
        a torch int64 tensor on the encoder's device -> (int16 tensor of the samples' units, int64
        offsets tensor), both on that device.  With out and out_off (contiguous int16 and int64 tensors
        on that device; 3 * units + 2 * texts and units + texts + 1 entries always suffice) the split
        runs once into them and views of them come back; without, a sizing call runs first."""
        import torch
        mode = lines_mode(mode)
        units, off = _units_tensors(units, off, 'split_lines_tensors', self.device)
        n = off.numel() - 1
        up = units.data_ptr() if units.numel() else None
        ns, need = ctypes.c_int64(), ctypes.c_int64()
        if out is not None and out_off is not None:
            if out.dtype != torch.int16 or out_off.dtype != torch.int64 or out.device != units.device or \
                    out_off.device != units.device or not (out.is_contiguous() and out_off.is_contiguous()):
                raise BpeError('split_lines_tensors takes contiguous int16 and int64 outputs on the device', ERR_ARG)
            _check(lib().bpe_encoder_split_lines_device(self._enc, mode, up, off.data_ptr(), n, out.data_ptr(),
                                                        out.numel(), out_off.data_ptr(), out_off.numel(),
                                                        ctypes.byref(ns), ctypes.byref(need)),
                   'bpe_encoder_split_lines_device')
            return out[:need.value], out_off[:ns.value + 1]
        rc = lib().bpe_encoder_split_lines_device(self._enc, mode, up, off.data_ptr(), n, None, 0, None, 0,
                                                  ctypes.byref(ns), ctypes.byref(need))
        # (the sizing call: too small even for no sample's one offset, so ERR_ARG with the numbers;
        # without a sample there was no text, and nothing else can be wrong)
        if rc != ERR_ARG or (ns.value <= 0 and n != 0):
            _check(rc, 'bpe_encoder_split_lines_device')
        out = torch.empty(max(need.value, 1), dtype=torch.int16, device=units.device)
        out_off = torch.zeros(ns.value + 1, dtype=torch.int64, device=units.device)
        torch.cuda.synchronize(units.device)
        _check(lib().bpe_encoder_split_lines_device(self._enc, mode, up, off.data_ptr(), n, out.data_ptr(),
                                                    out.numel(), out_off.data_ptr(), out_off.numel(),
                                                    ctypes.byref(ns), ctypes.byref(need)),
               'bpe_encoder_split_lines_device')
        return out[:need.value], out_off

    def lines_stats(self):
        s = LinesStats()
        _check(lib().bpe_encoder_get_lines_stats(self._enc, ctypes.byref(s)), 'bpe_encoder_get_lines_stats')
        return s.as_dict()

    def reset_lines_stats(self):
        _check(lib().bpe_encoder_reset_lines_stats(self._enc), 'bpe_encoder_reset_lines_stats')

    # skip-gram pairs (include/bpe.h "skip-gram pairs"): values -> (target, context) pairs on the device
    def skipgram_flat(self, vals, off, window=2):
        """The expansion alone (bpe_encoder_skipgram): texts vals[off[k]:off[k+1]] (int32 vector indices
        or ids) -> (targets int32, contexts int32, pair_off int64), the pairs of example/skip-gram.ts's
        loop over `window` values on each side.  The sizing call, then the real one."""
        vals = _i32(vals).ravel()
        off = np.ascontiguousarray(off, dtype=np.int64)
        src = vals if vals.size else np.zeros(1, np.int32)
        i64p = ctypes.POINTER(ctypes.c_int64)
        return _skipgram_host('bpe_encoder_skipgram', lambda t, c, cap, po: lib().bpe_encoder_skipgram(
            self._enc, src.ctypes.data, off.ctypes.data_as(i64p), len(off) - 1, int(window), t, c, cap, po),
            len(off) - 1)

    def skipgram(self, texts, window=2):
        """texts: a list of int sequences (encode_text's output) -> (targets, contexts, pair_off)."""
        parts = [_i32(t).ravel() for t in texts]
        off = np.zeros(len(parts) + 1, dtype=np.int64)
        np.cumsum([len(x) for x in parts], out=off[1:])
        vals = np.concatenate(parts) if parts and off[-1] else np.zeros(0, np.int32)
        return self.skipgram_flat(vals, off, window)

    def skipgram_tensors(self, vals, off, window=2, out=None):
        """Device form (bpe_encoder_skipgram_device): vals a torch int32 tensor and off a torch int64
        tensor on the encoder's device -> (targets, contexts, pair_off) tensors there: two int32 planes
        an nn.Embedding takes as they are, and int64 offsets.  out: a pair of contiguous int32 tensors
        on the device to write the planes into (views of them come back), else a sizing call runs
        first."""
        import torch
        if vals.dtype != torch.int32 or off.dtype != torch.int64:
            raise BpeError('skipgram_tensors takes int32 values and int64 offsets', ERR_ARG)
        if not (vals.is_cuda and off.is_cuda and vals.device.index == self.device and off.device.index == self.device):
            raise BpeError('skipgram_tensors takes tensors on the encoder\'s device', ERR_ARG)
        vals, off = vals.contiguous(), off.contiguous()
        vp = vals.data_ptr() if vals.numel() else None
        return _skipgram_device('bpe_encoder_skipgram_device', lambda t, c, cap, po, need: lib().bpe_encoder_skipgram_device(
            self._enc, vp, off.data_ptr(), off.numel() - 1, int(window), t, c, cap, po, need),
            off.numel() - 1, self.device, out)

    def skipgram_text_flat(self, units, off, window=2, kind='vectors'):
        """Texts units[off[k]:off[k+1]] (UTF-16 units) encoded and expanded on the device
        (bpe_skipgram_text_batch) -> (targets, contexts, pair_off)."""
        kind = self._KINDS[kind]
        units = np.ascontiguousarray(units, dtype=np.uint16).ravel()
        off = np.ascontiguousarray(off, dtype=np.int64)
        src = units if units.size else np.zeros(1, np.uint16)
        i64p = ctypes.POINTER(ctypes.c_int64)
        return _skipgram_host('bpe_skipgram_text_batch', lambda t, c, cap, po: lib().bpe_skipgram_text_batch(
            self._enc, kind, src.ctypes.data, off.ctypes.data_as(i64p), len(off) - 1, int(window), t, c, cap, po),
            len(off) - 1)

    def skipgram_text(self, texts, window=2, kind='vectors'):
        """texts: a list of str -> (targets, contexts, pair_off): encode_text, then skipgram."""
        units, off = _units_flat(texts)
        return self.skipgram_text_flat(units, off, window, kind)

    def skipgram_text_tensors(self, units, off, window=2, kind='vectors', out=None):
        """Device form (bpe_skipgram_text_batch_device): torch int16 or uint16 units and int64 offsets
        on the encoder's device -> (targets, contexts, pair_off) tensors there; no value touches the
        host.  out: as in skipgram_tensors."""
        kind = self._KINDS[kind]
        units, off = _units_tensors(units, off, 'skipgram_text_tensors', self.device)
        up = units.data_ptr() if units.numel() else None
        return _skipgram_device('bpe_skipgram_text_batch_device', lambda t, c, cap, po, need: lib().bpe_skipgram_text_batch_device(
            self._enc, kind, up, off.data_ptr(), off.numel() - 1, int(window), t, c, cap, po, need),
            off.numel() - 1, self.device, out)

    def skipgram_utf8(self, texts, off=None, window=2, kind='vectors'):
        """skipgram_text for UTF-8 (bpe_skipgram_utf8_batch): texts a list of bytes, or the flat form
        (uint8 array, int64 offsets) -> (targets, contexts, pair_off)."""
        kind = self._KINDS[kind]
        data, off = _utf8_flat(texts, off)
        src = data if data.size else np.zeros(1, np.uint8)
        i64p = ctypes.POINTER(ctypes.c_int64)
        return _skipgram_host('bpe_skipgram_utf8_batch', lambda t, c, cap, po: lib().bpe_skipgram_utf8_batch(
            self._enc, kind, src.ctypes.data, off.ctypes.data_as(i64p), len(off) - 1, int(window), t, c, cap, po),
            len(off) - 1)

    def skipgram_utf8_tensors(self, data, off, window=2, kind='vectors', out=None):
        """Device form (bpe_skipgram_utf8_batch_device): torch uint8 bytes and int64 offsets on the
        encoder's device -> (targets, contexts, pair_off) tensors there.  out: as in skipgram_tensors."""
        kind = self._KINDS[kind]
        data, off = _utf8_tensors(data, off, 'skipgram_utf8_tensors', self.device)
        dp = data.data_ptr() if data.numel() else None
        return _skipgram_device('bpe_skipgram_utf8_batch_device', lambda t, c, cap, po, need: lib().bpe_skipgram_utf8_batch_device(
            self._enc, kind, dp, off.data_ptr(), off.numel() - 1, int(window), t, c, cap, po, need),
            off.numel() - 1, self.device, out)

    def skipgram_stats(self):
        s = SkipgramStats()
        _check(lib().bpe_encoder_get_skipgram_stats(self._enc, ctypes.byref(s)), 'bpe_encoder_get_skipgram_stats')
        return s.as_dict()

    def reset_skipgram_stats(self):
        _check(lib().bpe_encoder_reset_skipgram_stats(self._enc), 'bpe_encoder_reset_skipgram_stats')


def _skipgram_host(what, call, n):
    """A skip-gram host form: call(targets, contexts, cap, pair_off) -> rc.  The sizing call, then the
    real one -> (targets int32, contexts int32, pair_off int64)."""
    off = np.zeros(n + 1, np.int64)
    po = off.ctypes.data_as(ctypes.POINTER(ctypes.c_int64))
    rc = call(None, None, 0, po)
    if rc == BPE_OK:   # (no pair to write)
        return np.zeros(0, np.int32), np.zeros(0, np.int32), off
    if rc != ERR_ARG or off[n] <= 0:
        _check(rc, what)
    t, c = np.empty(int(off[n]), np.int32), np.empty(int(off[n]), np.int32)
    _check(call(t.ctypes.data, c.ctypes.data, t.size, po), what)
    return t, c, off


def _skipgram_device(what, call, n, device, out=None):
    """A skip-gram device form: call(d_targets, d_contexts, cap, d_pair_off, needed) -> rc, into `out`
    (two contiguous int32 tensors on the device) or, after a sizing call, into new tensors
    -> (targets, contexts, pair_off) tensors."""
    import torch
    dev = torch.device('cuda', device)
    off = torch.zeros(n + 1, dtype=torch.int64, device=dev)
    need = ctypes.c_int64()
    torch.cuda.synchronize(dev)   # (encoders and contexts run on streams of their own)
    if out is None:
        rc = call(None, None, 0, off.data_ptr(), ctypes.byref(need))
        if rc == BPE_OK:   # (no pair to write)
            return (torch.zeros(0, dtype=torch.int32, device=dev), torch.zeros(0, dtype=torch.int32, device=dev), off)
        if rc != ERR_ARG or need.value <= 0:
            _check(rc, what)
        t = torch.empty(need.value, dtype=torch.int32, device=dev)
        c = torch.empty(need.value, dtype=torch.int32, device=dev)
    else:
        t, c = out
        for x in (t, c):
            if x.dtype != torch.int32 or not x.is_cuda or x.device.index != device or not x.is_contiguous():
                raise BpeError('%s takes two contiguous int32 tensors on the device as out' % what, ERR_ARG)
    cap = min(t.numel(), c.numel())
    torch.cuda.synchronize(dev)
    _check(call(t.data_ptr() if cap else None, c.data_ptr() if cap else None, cap, off.data_ptr(), ctypes.byref(need)),
           what)
    return t[:need.value], c[:need.value], off


def lines_mode(mode):
    """'trim' | 'keep' | 'file' (or the LINES_* constant) -> the constant; anything else is an error."""
    try:
        return _LINES_MODES[mode]
    except (KeyError, TypeError):
        raise BpeError('unknown lines mode %r (trim, keep or file)' % (mode,), ERR_ARG)


def _units_flat(texts):
    """A list of str (or unit arrays) as (uint16 array, int64 offsets)."""
    parts = [_units(t) for t in texts]
    off = np.zeros(len(parts) + 1, dtype=np.int64)
    np.cumsum([len(x) for x in parts], out=off[1:])
    units = np.concatenate(parts).astype(np.uint16) if parts and off[-1] else np.zeros(0, np.uint16)
    return units, off


def _units_tensors(units, off, what, device=None):
    """Checks a device batch of UTF-16 units: a torch int16 or uint16 tensor and int64 offsets on one
    device (`device`: which one)."""
    import torch
    if units.dtype not in (torch.int16, getattr(torch, 'uint16', torch.int16)) or off.dtype != torch.int64:
        raise BpeError('%s takes int16 or uint16 units and int64 offsets' % what, ERR_ARG)
    if not (units.is_cuda and off.is_cuda and units.device == off.device) or \
            (device is not None and units.device.index != device):
        raise BpeError('%s takes tensors on the device of the call' % what, ERR_ARG)
    units, off = units.contiguous(), off.contiguous()
    torch.cuda.synchronize(units.device)   # (contexts and encoders run on streams of their own)
    return units, off


def _utf8_flat(texts, off):
    """A batch of UTF-8 texts as (uint8 array, int64 offsets): a list of bytes-like objects
    (off None), or the flat form as it is."""
    if off is not None:
        return np.ascontiguousarray(texts, dtype=np.uint8).ravel(), np.ascontiguousarray(off, dtype=np.int64)
    parts = [bytes(t) for t in texts]
    off = np.zeros(len(parts) + 1, dtype=np.int64)
    np.cumsum([len(x) for x in parts], out=off[1:])
    return np.frombuffer(b''.join(parts), dtype=np.uint8), off


def _utf8_tensors(data, off, what, device=None):
    """Checks a device batch: a torch uint8 tensor (a view at any byte offset is fine) and int64
    offsets on one device (`device`: which one)."""
    import torch
    if data.dtype != torch.uint8 or off.dtype != torch.int64:
        raise BpeError('%s takes uint8 bytes and int64 offsets' % what, ERR_ARG)
    if not (data.is_cuda and off.is_cuda and data.device == off.device) or \
            (device is not None and data.device.index != device):
        raise BpeError('%s takes tensors on the device of the call' % what, ERR_ARG)
    data, off = data.contiguous(), off.contiguous()
    torch.cuda.synchronize(data.device)   # (contexts and encoders run on streams of their own)
    return data, off


def _units(x):
    """A token's chars as UTF-16 code units: a str (lone surrogates kept) or an array of units."""
    if isinstance(x, str):
        return np.frombuffer(x.encode('utf-16-le', 'surrogatepass'), dtype='<u2')
    return np.ascontiguousarray(x, dtype=np.uint16).ravel()


def units_to_str(units):
    """UTF-16 code units -> str, lone surrogates kept (as a JS string holds them)."""
    return np.ascontiguousarray(units, dtype='<u2').tobytes().decode('utf-16-le', 'surrogatepass')


class Decoder:
    """decodeVector / decodeTokens (core.ts:447-471) for batches of texts (bpe_decoder_*,
    include/bpe.h): the vocabulary lives on the device as a blob of UTF-16 units and one record per
    token id; a call expands vector indices or token ids into units there (csrc/bpe_decode.hip).
    No CPU fallback."""

    _KINDS = {'ids': DECODE_IDS, 'tokens': DECODE_IDS, 'vectors': DECODE_VECTORS,
              DECODE_IDS: DECODE_IDS, DECODE_VECTORS: DECODE_VECTORS}

    def __init__(self, device=0):
        p = ctypes.c_void_p()
        _check(lib().bpe_decoder_create(ctypes.byref(p), int(device)), 'bpe_decoder_create')
        self._dec = p
        self.device = int(device)

    def close(self):
        if getattr(self, '_dec', None):
            lib().bpe_decoder_destroy(self._dec)
            self._dec = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def clear(self):
        _check(lib().bpe_decoder_clear(self._dec), 'bpe_decoder_clear')

    def add_tokens(self, tokens):
        """Appends char tokens: each a str (encoded with surrogatepass, so lone surrogates
        survive) or an array of UTF-16 units."""
        parts = [_units(t) for t in tokens]
        off = np.zeros(len(parts) + 1, dtype=np.int64)
        np.cumsum([len(x) for x in parts], out=off[1:])
        units = np.ascontiguousarray(np.concatenate(parts), dtype=np.uint16) if off[-1] \
            else np.zeros(1, np.uint16)
        _check(lib().bpe_decoder_add_tokens(self._dec, units.ctypes.data,
                                            off.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)),
                                            len(parts)), 'bpe_decoder_add_tokens')

    def add_merges(self, merges):
        """Appends merged tokens from (a, b, c) triples: chars[c] = chars[a] + chars[b]."""
        abc = _i32(np.asarray(merges, dtype=np.int32).reshape(-1))
        _check(lib().bpe_decoder_add_merges(self._dec, abc.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)),
                                            len(abc) // 3), 'bpe_decoder_add_merges')

    def num_tokens(self):
        """(token count, UTF-16 units of all tokens' chars)."""
        n, u = ctypes.c_int32(), ctypes.c_int64()
        _check(lib().bpe_decoder_num_tokens(self._dec, ctypes.byref(n), ctypes.byref(u)),
               'bpe_decoder_num_tokens')
        return n.value, u.value

    def set_vector_index(self, from_vector_index):
        """from_vector_index of compactVectorIndex (core.ts:222-241); None drops the index."""
        if from_vector_index is None:
            _check(lib().bpe_decoder_set_vector_index(self._dec, None, 0), 'bpe_decoder_set_vector_index')
            return
        a = _i32(from_vector_index).ravel()
        buf = a if a.size else np.zeros(1, np.int32)
        _check(lib().bpe_decoder_set_vector_index(self._dec, buf.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)),
                                                  a.size), 'bpe_decoder_set_vector_index')

    def decode_flat(self, vals, off, kind='vectors'):
        """Flat form: texts vals[off[k]:off[k+1]] -> (units uint16, out_off int64).  The sizing
        call, then the real one."""
        kind = self._KINDS[kind]
        vals = _i32(vals).ravel()
        off = np.ascontiguousarray(off, dtype=np.int64)
        n = len(off) - 1
        src = vals if vals.size else np.zeros(1, np.int32)
        i32p, i64p = ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_int64)
        out_off = np.zeros(n + 1, dtype=np.int64)
        rc = lib().bpe_decode_batch(self._dec, kind, src.ctypes.data_as(i32p), off.ctypes.data_as(i64p), n,
                                    None, 0, out_off.ctypes.data_as(i64p))
        if rc == BPE_OK:   # (nothing to write)
            return np.zeros(0, np.uint16), out_off
        if rc != ERR_ARG or out_off[n] <= 0:
            _check(rc, 'bpe_decode_batch')
        units = np.empty(int(out_off[n]), dtype=np.uint16)
        _check(lib().bpe_decode_batch(self._dec, kind, src.ctypes.data_as(i32p), off.ctypes.data_as(i64p), n,
                                      units.ctypes.data, units.size, out_off.ctypes.data_as(i64p)),
               'bpe_decode_batch')
        return units, out_off

    def decode(self, texts, kind='vectors'):
        """texts: a list of vectors (or id sequences, kind='ids') -> list of str."""
        lens = [len(t) for t in texts]
        off = np.zeros(len(texts) + 1, dtype=np.int64)
        np.cumsum(lens, out=off[1:])
        vals = np.concatenate([np.asarray(t, dtype=np.int32) for t in texts]) if texts and off[-1] \
            else np.zeros(0, np.int32)
        units, oo = self.decode_flat(vals, off, kind)
        raw = units.astype('<u2', copy=False).tobytes()
        return [raw[2 * oo[k]:2 * oo[k + 1]].decode('utf-16-le', 'surrogatepass')
                for k in range(len(texts))]

    def decode_tensors(self, vals, off, kind='vectors'):
        """Device form (bpe_decode_batch_device): vals a torch int32 tensor and off a torch int64
        tensor on the decoder's device -> (int16 tensor of the units, int64 offsets tensor), both on
        that device."""
        import torch
        kind = self._KINDS[kind]
        if vals.dtype != torch.int32 or off.dtype != torch.int64:
            raise BpeError('decode_tensors takes int32 values and int64 offsets', ERR_ARG)
        if not (vals.is_cuda and off.is_cuda and vals.device.index == self.device
                and off.device.index == self.device):
            raise BpeError('decode_tensors takes tensors on the decoder\'s device', ERR_ARG)
        vals, off = vals.contiguous(), off.contiguous()
        n = off.numel() - 1
        out_off = torch.zeros(n + 1, dtype=torch.int64, device=vals.device)
        torch.cuda.synchronize(vals.device)   # (the decoder runs on a stream of its own)
        need = ctypes.c_int64()
        vp = vals.data_ptr() if vals.numel() else None
        rc = lib().bpe_decode_batch_device(self._dec, kind, vp, off.data_ptr(), n, None, 0,
                                           out_off.data_ptr(), ctypes.byref(need))
        if rc == BPE_OK:
            return torch.zeros(0, dtype=torch.int16, device=vals.device), out_off
        if rc != ERR_ARG or need.value <= 0:
            _check(rc, 'bpe_decode_batch_device')
        units = torch.empty(need.value, dtype=torch.int16, device=vals.device)
        torch.cuda.synchronize(vals.device)
        _check(lib().bpe_decode_batch_device(self._dec, kind, vp, off.data_ptr(), n, units.data_ptr(),
                                             units.numel(), out_off.data_ptr(), ctypes.byref(need)),
               'bpe_decode_batch_device')
        return units, out_off

    # ---- text out as UTF-8 (include/bpe.h "text out as UTF-8", csrc/bpe_utf8_out.hip.h) ----

    def _sized_host(self, what, call, n):
        """The sizing call, then the real one: call(out_ptr, cap, out_off_ptr) -> rc."""
        out_off = np.zeros(n + 1, dtype=np.int64)
        i64p = ctypes.POINTER(ctypes.c_int64)
        rc = call(None, 0, out_off.ctypes.data_as(i64p))
        if rc == BPE_OK:   # (nothing to write)
            return np.zeros(0, np.uint8), out_off
        if rc != ERR_ARG or out_off[-1] <= 0:
            _check(rc, what)
        out = np.empty(int(out_off[-1]), dtype=np.uint8)
        _check(call(out.ctypes.data, out.size, out_off.ctypes.data_as(i64p)), what)
        return out, out_off

    def _sized_device(self, what, call, n, device):
        """... on the device: call(out_ptr, cap, out_off_ptr, needed_ref) -> rc."""
        import torch
        out_off = torch.zeros(n + 1, dtype=torch.int64, device=device)
        need = ctypes.c_int64()
        torch.cuda.synchronize(device)   # (the decoder runs on a stream of its own)
        rc = call(None, 0, out_off.data_ptr(), ctypes.byref(need))
        if rc == BPE_OK:
            return torch.zeros(0, dtype=torch.uint8, device=device), out_off
        if rc != ERR_ARG or need.value <= 0:
            _check(rc, what)
        out = torch.empty(need.value, dtype=torch.uint8, device=device)
        torch.cuda.synchronize(device)
        _check(call(out.data_ptr(), out.numel(), out_off.data_ptr(), ctypes.byref(need)), what)
        return out, out_off

    def utf16_to_utf8(self, texts_or_units, off=None):
        """The transcode alone (bpe_decoder_utf16_to_utf8): a list of str or unit arrays (off None),
        or the flat form (uint16 units, int64 offsets) -> (bytes uint8, out_off int64), each text
        encoded as Node's Buffer.from(text) encodes it (lone surrogates: EF BF BD)."""
        if off is None:
            parts = [_units(t) for t in texts_or_units]
            off = np.zeros(len(parts) + 1, dtype=np.int64)
            np.cumsum([len(x) for x in parts], out=off[1:])
            units = np.ascontiguousarray(np.concatenate(parts), dtype=np.uint16) if off[-1] else np.zeros(1, np.uint16)
        else:
            units = np.ascontiguousarray(texts_or_units, dtype=np.uint16).ravel()
            off = np.ascontiguousarray(off, dtype=np.int64)
        n = len(off) - 1
        src = units if units.size else np.zeros(1, np.uint16)
        i64p = ctypes.POINTER(ctypes.c_int64)

        def call(out, cap, oo):
            return lib().bpe_decoder_utf16_to_utf8(self._dec, src.ctypes.data, off.ctypes.data_as(i64p), n, out, cap, oo)
        return self._sized_host('bpe_decoder_utf16_to_utf8', call, n)

    def utf16_to_utf8_tensors(self, units, off):
        """Device form (bpe_decoder_utf16_to_utf8_device): units a torch int16 (or uint16) tensor, a
        view at any unit offset is fine, and off a torch int64 tensor on the decoder's device ->
        (uint8 tensor of the bytes, int64 offsets tensor) on that device."""
        import torch
        if units.dtype not in (torch.int16, getattr(torch, 'uint16', torch.int16)) or off.dtype != torch.int64:
            raise BpeError('utf16_to_utf8_tensors takes int16 units and int64 offsets', ERR_ARG)
        if not (units.is_cuda and off.is_cuda and units.device.index == self.device
                and off.device.index == self.device):
            raise BpeError('utf16_to_utf8_tensors takes tensors on the decoder\'s device', ERR_ARG)
        units, off = units.contiguous(), off.contiguous()
        n = off.numel() - 1
        up = units.data_ptr() if units.numel() else None

        def call(out, cap, oo, need):
            return lib().bpe_decoder_utf16_to_utf8_device(self._dec, up, off.data_ptr(), n, out, cap, oo, need)
        return self._sized_device('bpe_decoder_utf16_to_utf8_device', call, n, units.device)

    def decode_utf8_flat(self, vals, off, kind='vectors'):
        """Flat form (bpe_decode_utf8_batch): texts vals[off[k]:off[k+1]] -> (bytes uint8, out_off
        int64).  The sizing call, then the real one."""
        kind = self._KINDS[kind]
        vals = _i32(vals).ravel()
        off = np.ascontiguousarray(off, dtype=np.int64)
        n = len(off) - 1
        src = vals if vals.size else np.zeros(1, np.int32)
        i32p, i64p = ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_int64)

        def call(out, cap, oo):
            return lib().bpe_decode_utf8_batch(self._dec, kind, src.ctypes.data_as(i32p), off.ctypes.data_as(i64p), n,
                                               out, cap, oo)
        return self._sized_host('bpe_decode_utf8_batch', call, n)

    def decode_utf8(self, texts, kind='vectors'):
        """texts: a list of vectors (or id sequences, kind='ids') -> list of bytes."""
        lens = [len(t) for t in texts]
        off = np.zeros(len(texts) + 1, dtype=np.int64)
        np.cumsum(lens, out=off[1:])
        vals = np.concatenate([np.asarray(t, dtype=np.int32) for t in texts]) if texts and off[-1] \
            else np.zeros(0, np.int32)
        out, oo = self.decode_utf8_flat(vals, off, kind)
        raw = out.tobytes()
        return [raw[oo[k]:oo[k + 1]] for k in range(len(texts))]

    def decode_utf8_tensors(self, vals, off, kind='vectors'):
        """Device form (bpe_decode_utf8_batch_device): vals a torch int32 tensor and off a torch int64
        tensor on the decoder's device -> (uint8 tensor of the bytes, int64 offsets tensor), both on
        that device."""
        import torch
        kind = self._KINDS[kind]
        if vals.dtype != torch.int32 or off.dtype != torch.int64:
            raise BpeError('decode_utf8_tensors takes int32 values and int64 offsets', ERR_ARG)
        if not (vals.is_cuda and off.is_cuda and vals.device.index == self.device
                and off.device.index == self.device):
            raise BpeError('decode_utf8_tensors takes tensors on the decoder\'s device', ERR_ARG)
        vals, off = vals.contiguous(), off.contiguous()
        n = off.numel() - 1
        vp = vals.data_ptr() if vals.numel() else None

        def call(out, cap, oo, need):
            return lib().bpe_decode_utf8_batch_device(self._dec, kind, vp, off.data_ptr(), n, out, cap, oo, need)
        return self._sized_device('bpe_decode_utf8_batch_device', call, n, vals.device)

    def utf8_stats(self):
        s = Utf8Stats()
        _check(lib().bpe_decoder_get_utf8_stats(self._dec, ctypes.byref(s)), 'bpe_decoder_get_utf8_stats')
        return s.as_dict()

    def reset_utf8_stats(self):
        _check(lib().bpe_decoder_reset_utf8_stats(self._dec), 'bpe_decoder_reset_utf8_stats')

    def stats(self):
        s = DecoderStats()
        _check(lib().bpe_decoder_get_stats(self._dec, ctypes.byref(s)), 'bpe_decoder_get_stats')
        return s.as_dict()

    def reset_stats(self):
        _check(lib().bpe_decoder_reset_stats(self._dec), 'bpe_decoder_reset_stats')


def encode_samples(samples, merges, len16=None, device=0):
    """Batch encoding with a trained merge list (encodeToCode, core.ts:392-409, for many texts at
    once): the device encoder (bpe_encode_batch) — the merge-rank kernel for samples up to
    ENCODE_LDS_TOKENS tokens, apply-only replay passes for longer ones.  merges: (a, b, c) triples
    in list order.  (len16 is accepted for the older signature; encoding never reads it.)"""
    enc = Encoder(device, merges)
    try:
        return [x.tolist() for x in enc.encode([np.asarray(s, dtype=np.int32) for s in samples])]
    finally:
        enc.close()
