#!/usr/bin/env python3
"""Kernel time of the dropout encoder (bpe_encode_dropout_batch, csrc/bpe_dropout.hip.h) beside the
plain one (bpe_encode_batch) on the `bench.py --full` encoder batch: 100 000 texts of 16-1024 chars
under the merges of tools/encode_bench.py's training run.

For every p in {0, 0.1, 0.5} and S in {1, 4}: ten rounds after one warm-up round, each round one
encode_dropout_flat call and one encode_flat call of the same batch (alternating, so both see the
same machine state); the best round of each is reported: kernel time from the encoders' HIP events
(per sample for the dropout kernel), end-to-end time of the call, and the ratio of the dropout
kernel's time per sample to the plain kernel's.  p = 0 is checked against encode_flat's output.
One JSON line per (p, S) on stdout and appended to --out.

A batch of this size goes through bpe_encode_batch in three groups, whose kernel time spans each
group's pack kernels too; the dropout call is one launch per shape and its kernel time stops before
the pack.  --one-group sets BPE_ENCODE_ONE_GROUP so that bpe_encode_batch also runs as one group
with its pack outside the events: the like-for-like kernel comparison.

Usage: tools/encode_dropout_bench.py [--mib 256] [--merges 8000] [--texts 100000] [--rounds 10] [--one-group] [--out FILE]
"""
import argparse
import importlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
if '--one-group' in sys.argv:   # (read by the library at the call)
    os.environ['BPE_ENCODE_ONE_GROUP'] = '1'
pkg = importlib.import_module('bpe-tokenizer_amd')


def timed(call, stats, reset):
    """-> (kernel ms by the encoder's events, end-to-end ms, the call's result)"""
    reset()
    t0 = time.perf_counter()
    out = call()
    e2e = time.perf_counter() - t0
    return stats()['kernel_ms'], e2e * 1e3, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--mib', type=int, default=256)
    ap.add_argument('--merges', type=int, default=8000)
    ap.add_argument('--texts', type=int, default=100000)
    ap.add_argument('--min', type=int, default=16)
    ap.add_argument('--max', type=int, default=1024)
    ap.add_argument('--rounds', type=int, default=10)
    ap.add_argument('--one-group', action='store_true')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'encode_dropout_bench.jsonl'))
    a = ap.parse_args()

    n = a.mib << 20
    lens = np.random.default_rng(5).integers(a.min, a.max + 1, size=a.texts)
    need = int(lens.sum())
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
    np.cumsum(lens, out=off[1:])
    off = np.minimum(off, ids.size)
    tokens = int(off[-1])

    enc = pkg.Encoder(0, merges)
    for p in (0.0, 0.1, 0.5):
        for S in (1, 4):
            best = {'drop_k': np.inf, 'drop_e2e': np.inf, 'enc_k': np.inf, 'enc_e2e': np.inf}
            for rnd in range(a.rounds + 1):   # (round 0 warms both up)
                dk, de, (dout, doo) = timed(lambda: enc.encode_dropout_flat(ids, off, p, S, seed=rnd), enc.dropout_stats,
                                            enc.reset_dropout_stats)
                ek, ee, (eout, eoo) = timed(lambda: enc.encode_flat(ids, off), enc.stats, enc.reset_stats)
                if rnd == 0:
                    continue
                best = {'drop_k': min(best['drop_k'], dk), 'drop_e2e': min(best['drop_e2e'], de),
                        'enc_k': min(best['enc_k'], ek), 'enc_e2e': min(best['enc_e2e'], ee)}
            same = None
            if p == 0.0:   # every sample is encode's output
                rep_len = np.repeat(np.diff(eoo), S)
                same = bool(np.array_equal(np.diff(doo), rep_len) and np.array_equal(
                    dout, eout[np.repeat(np.repeat(eoo[:-1], S) - doo[:-1], rep_len) + np.arange(int(doo[-1]))]))
            res = {'what': 'k_encode_drop beside k_encode on %d texts of %d-%d chars, %d merges; best of %d warmed, '
                           'alternating calls' % (a.texts, a.min, a.max, len(merges), a.rounds),
                   'encode_one_group': a.one_group, 'p': p, 'samples': S, 'tokens_in': tokens, 'tokens_out_dropout': int(doo[-1]), 'tokens_out_encode': int(eoo[-1]),
                   'dropout_kernel_ms': best['drop_k'], 'dropout_kernel_ms_per_sample': best['drop_k'] / S,
                   'dropout_e2e_ms': best['drop_e2e'], 'encode_kernel_ms': best['enc_k'], 'encode_e2e_ms': best['enc_e2e'],
                   'dropout_kernel_tokens_per_s': tokens * S / (best['drop_k'] * 1e-3),
                   'encode_kernel_tokens_per_s': tokens / (best['enc_k'] * 1e-3),
                   'kernel_ratio_per_sample': best['drop_k'] / S / best['enc_k'],
                   'p0_equals_encode': same}
            line = json.dumps(res)
            print(line, flush=True)
            with open(a.out, 'a') as f:
                f.write(line + '\n')
    enc.close()


if __name__ == '__main__':
    main()
