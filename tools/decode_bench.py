#!/usr/bin/env python3
"""Throughput of the device decoder (bpe_decode_batch, csrc/bpe_decode.hip): decodeTokens /
decodeVector (core.ts:447-471) of a batch of encoded texts back to UTF-16 units.

The batch is the encoder bench's output (tools/encode_bench.py): merges from mergeUntil({min_weight:
2, max_iterations: M}) on MiB of a synthetic corpus, a later stretch of the same stream cut into
texts of [min, max] chars, encoded by the device encoder.  Its ids are decoded as token ids, and as
vector indices through the compact index of a table whose tokens are all live.  Prints one JSON
line per kind:
  - kernel time (HIP events around the launches, bpe_decoder_get_stats), the bytes the pipeline
    moves through HBM by its shape (4 B per value read twice, 2 B per unit written; the tables are
    L2 reads) and their share of the HBM bandwidth (8 TB/s spec peak, 6.29 TB/s measured copy rate:
    MI355X_MICROARCH.md);
  - end-to-end time of the host form (copies up, kernels, copies down), without the sizing call;
  - cpu_numpy: a vectorised numpy decode of the same batch on the host (np.repeat of the record
    offsets plus an arange, one fancy-index of the blob), whose output must equal the device's.

Usage: tools/decode_bench.py [--corpus uniform|zipf] [--mib 256] [--merges 8000] [--texts 100000]
                             [--min 16] [--max 1024] [--reps 5]
"""
import argparse
import ctypes
import importlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
pkg = importlib.import_module('bpe-tokenizer_amd')

HBM_PEAK_GBS = 8000.0      # MI355X HBM3E spec peak (MI355X_MICROARCH.md)
HBM_COPY_GBS = 6290.0      # ... and the measured float4 copy rate


def numpy_decode(vals, off, blob, start, lens, index=None):
    ids = vals if index is None else index[vals]
    l = lens[ids].astype(np.int64)
    ends = np.cumsum(l)
    src = np.repeat(start[ids].astype(np.int64) - (ends - l), l) + np.arange(int(ends[-1]) if len(ends) else 0)
    return blob[src], np.concatenate([[0], ends])[off - off[0]]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--corpus', default='uniform')
    ap.add_argument('--mib', type=int, default=256)
    ap.add_argument('--merges', type=int, default=8000)
    ap.add_argument('--texts', type=int, default=100000)
    ap.add_argument('--min', type=int, default=16)
    ap.add_argument('--max', type=int, default=1024)
    ap.add_argument('--reps', type=int, default=5)
    a = ap.parse_args()

    n = a.mib << 20
    rng = np.random.default_rng(5)
    text_lens = rng.integers(a.min, a.max + 1, size=a.texts)
    need = int(text_lens.sum())
    if a.corpus == 'zipf':
        data = pkg.synth_zipf(n + need, seed=12345)
        train, rest = data[:n], data[n:n + need]
    else:
        train = pkg.synth_latin1(n, seed=12345, A=256)
        rest = pkg.synth_latin1(need, seed=12345, A=256, skip=n)
    e = pkg.Engine(0)
    cmap, n_tok, _ = e.add_latin1(train, sample_bytes=1 << 20)
    e.set_mode('incremental')
    got = e.merge_until(0, 2, a.merges)
    e.close()
    merges = np.asarray([(x, y, n_tok + k) for k, (x, y, _w) in enumerate(got)], np.int32)
    ids = cmap[rest]
    ids = ids[ids >= 0].astype(np.int32)
    off = np.zeros(a.texts + 1, np.int64)
    np.cumsum(text_lens, out=off[1:])
    off = np.minimum(off, ids.size)
    enc = pkg.Encoder(0, merges)
    vals, voff = enc.encode_flat(ids, off)
    enc.close()
    vals = np.ascontiguousarray(vals)

    # the vocabulary: one latin1 char per base token, then the merges
    seen = np.nonzero(cmap >= 0)[0]
    byte_of = np.zeros(n_tok, np.uint16)
    byte_of[cmap[seen]] = seen
    dec = pkg.Decoder(0)
    dec.add_tokens([byte_of[i:i + 1] for i in range(n_tok)])
    dec.add_merges(merges)
    n_tokens, n_units = dec.num_tokens()
    # the same tables on the host for the numpy leg
    chars = [byte_of[i:i + 1] for i in range(n_tok)]
    for x, y, _c in merges:
        chars.append(np.concatenate([chars[x], chars[y]]))
    lens = np.asarray([len(c) for c in chars], np.int64)
    start = np.concatenate([[0], np.cumsum(lens)[:-1]])
    blob = np.concatenate(chars)
    index = np.arange(n_tokens, dtype=np.int32)     # every token live: the compact index is 0..n-1

    i32p, i64p = ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_int64)
    for kind in ('ids', 'vectors'):
        if kind == 'vectors':
            dec.set_vector_index(index)
        units, oo = dec.decode_flat(vals, voff, kind)          # warmup, and the sizes
        out = np.empty(units.size, np.uint16)
        dec.reset_stats()
        t0 = time.perf_counter()
        for _ in range(a.reps):
            rc = pkg.lib().bpe_decode_batch(dec._dec, pkg.Decoder._KINDS[kind], vals.ctypes.data_as(i32p),
                                            voff.ctypes.data_as(i64p), a.texts, out.ctypes.data, out.size,
                                            oo.ctypes.data_as(i64p))
            assert rc == 0, pkg.last_error()
        e2e = (time.perf_counter() - t0) / a.reps
        st = dec.stats()
        kern = st['kernel_ms'] / a.reps / 1e3
        t0 = time.perf_counter()
        want, want_off = numpy_decode(vals, voff, blob, start, lens, index if kind == 'vectors' else None)
        t_cpu = time.perf_counter() - t0
        same = bool(np.array_equal(want, out) and np.array_equal(want_off, oo))
        hbm_bytes = 8 * vals.size + 2 * out.size
        res = {
            'what': 'decode of a batch of encoded texts to UTF-16 units on the device decoder',
            'kind': kind, 'corpus': a.corpus, 'train_mib': a.mib, 'merges': int(len(merges)),
            'texts': a.texts, 'text_chars': [a.min, a.max], 'values_in': int(vals.size),
            'units_out': int(out.size), 'vocab_tokens': n_tokens, 'vocab_units': n_units,
            'kernel_ms': kern * 1e3, 'hbm_bytes': hbm_bytes, 'kernel_gbs': hbm_bytes / kern / 1e9,
            'frac_hbm_peak': hbm_bytes / kern / 1e9 / HBM_PEAK_GBS,
            'frac_hbm_copy_rate': hbm_bytes / kern / 1e9 / HBM_COPY_GBS,
            'kernel_units_per_s': out.size / kern, 'e2e_ms': e2e * 1e3, 'e2e_units_per_s': out.size / e2e,
            'cpu_numpy': {'kind': 'vectorised numpy decode, one thread', 's': t_cpu,
                          'units_per_s': out.size / t_cpu},
            'identical_to_cpu': same,
        }
        print(json.dumps(res), flush=True)
    dec.close()


if __name__ == '__main__':
    main()
