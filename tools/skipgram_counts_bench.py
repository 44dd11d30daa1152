#!/usr/bin/env python3
"""What the skip-gram pair counts cost (csrc/bpe_skipgram_counts.hip.h: values -> every distinct
(target, context) pair with its count, on the device) beside the pair expansion of the same input.

The workloads are tools/skipgram_bench.py's: the encoder output of its batch as vectors (the ids
through a compact index) at windows 2 and 5, one text of 2^24 values at window 2, and the trained
corpus at window 2.  One JSON line per workload, printed and written to
profiles/skipgram_counts_bench.jsonl:
  - P, U and lds_overflow (bpe_skipgram_counts_stats);
  - the kernels' time (HIP events: clearing the accumulator, count, sym, census, scan, emit) as the
    best and the worst of --reps runs, per value, and the pair expansion's kernel time in the same run;
  - the whole call from device buffers (into preallocated planes, and with the sizing call) and from
    host buffers;
  - the host route to the same counts (numpy `unique` over the expanded pairs) and whether every
    route's output was identical.

Usage: tools/skipgram_counts_bench.py [--texts 100000] [--min 16] [--max 1024] [--reps 5] [--merges 100]
"""
import argparse
import importlib
import json
import os
import sys

import numpy as np

import torch  # (before libbpe loads: PyTorch's HIP runtime must be the process's first)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))
pkg = importlib.import_module('bpe-tokenizer_amd')
from utf8_bench import best  # noqa: E402


def numpy_counts(t, c, dim):
    """The host route: `unique` over the expanded pairs' keys."""
    k, n = np.unique(t.astype(np.int64) * dim + c, return_counts=True)
    return (k // dim).astype(np.int32), (k % dim).astype(np.int32), n.astype(np.int64)


def identical(a, b):
    return bool(all(np.array_equal(x.cpu().numpy() if hasattr(x, 'cpu') else x, y) for x, y in zip(a, b)))


def measure(name, enc, vals, off, w, dim, reps, dev):
    d_vals, d_off = torch.from_numpy(vals).to(dev), torch.from_numpy(off).to(dev)
    got = enc.skipgram_counts_tensors(d_vals, d_off, w, dim)   # warm-up; sizes the planes
    out = tuple(torch.empty_like(x) for x in got)
    k_ms = []
    for _ in range(reps):
        enc.reset_skipgram_counts_stats()
        enc.skipgram_counts_tensors(d_vals, d_off, w, dim, out=out)
        st = enc.skipgram_counts_stats()
        k_ms.append(st['kernel_ms'])
    _, t_dev_out = best(lambda: enc.skipgram_counts_tensors(d_vals, d_off, w, dim, out=out), reps)
    _, t_dev = best(lambda: enc.skipgram_counts_tensors(d_vals, d_off, w, dim), reps)
    host, t_host = best(lambda: enc.skipgram_counts(vals, off, w, dim), reps)
    # the pair expansion of the same input in the same run, and the host route over its pairs
    pt, pc, _po = enc.skipgram_tensors(d_vals, d_off, w)
    planes = (torch.empty_like(pt), torch.empty_like(pc))
    p_ms = []
    for _ in range(reps):
        enc.reset_skipgram_stats()
        enc.skipgram_tensors(d_vals, d_off, w, out=planes)
        p_ms.append(enc.skipgram_stats()['kernel_ms'])
    ht, hc = pt.cpu().numpy(), pc.cpu().numpy()
    del pt, pc, planes
    want, t_np = best(lambda: numpy_counts(ht, hc, dim), 1)
    return {'what': 'skip-gram pair counts: values counted into distinct (target, context) pairs on the device',
            'workload': name, 'window': w, 'dim': dim, 'texts': len(off) - 1, 'values': int(len(vals)),
            'pairs_counted': st['pairs_counted'], 'distinct': st['distinct_out'], 'lds_overflow': st['lds_overflow'],
            'kernel_ms': round(min(k_ms), 3), 'kernel_ms_worst': round(max(k_ms), 3),
            'kernel_ns_per_value': min(k_ms) * 1e6 / len(vals), 'kernel_ns_per_value_worst': max(k_ms) * 1e6 / len(vals),
            'pairs_expand_kernel_ms': round(min(p_ms), 3),
            'device_into_planes_ms': round(t_dev_out * 1e3, 3), 'device_with_sizing_ms': round(t_dev * 1e3, 3),
            'host_ms': round(t_host * 1e3, 3), 'numpy_unique_over_pairs_ms': round(t_np * 1e3, 3),
            'identical': identical(out, want) and identical(got, want) and identical(host, want)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--texts', type=int, default=100000)
    ap.add_argument('--min', type=int, default=16)
    ap.add_argument('--max', type=int, default=1024)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--merges', type=int, default=100)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'skipgram_counts_bench.jsonl'))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit('skipgram_counts_bench needs a HIP device')
    dev = torch.device('cuda', 0)
    rng = np.random.default_rng(5)
    text_lens = rng.integers(a.min, a.max + 1, size=a.texts)
    src = pkg.synth_latin1(int(text_lens.sum()), seed=12345, A=256, skip=256 << 20)
    data = (src % 95 + 0x20).astype(np.uint8)           # printable ASCII: the bytes are the chars
    boff = np.zeros(a.texts + 1, np.int64)
    np.cumsum(text_lens, out=boff[1:])

    eng = pkg.Engine(0)
    new_chars, _ = eng.add_utf8_batch(data, boff)
    merges = eng.merge_until(0, 2, a.merges)
    abc = [(m[0], m[1], len(new_chars) + i) for i, m in enumerate(merges)]
    enc = pkg.Encoder(0, abc)
    enc.set_chars({int(cp): i for i, cp in enumerate(new_chars)})
    ids, ioff = enc.encode_utf8(data, boff, 'ids')
    # vectors: the ids that occur, ranked
    live, vec = np.unique(ids, return_inverse=True)
    vec = np.ascontiguousarray(vec, np.int32)
    dim = int(len(live))

    lines = []
    for w in (2, 5):
        lines.append(measure('encoder_output', enc, vec, ioff, w, dim, a.reps, dev))
        print(json.dumps(lines[-1]), flush=True)
    one = (np.arange(1 << 24, dtype=np.int64) * 2654435761 % 50021 % dim).astype(np.int32)
    lines.append(measure('one_text', enc, one, np.asarray([0, 1 << 24], np.int64), 2, dim, a.reps, dev))
    print(json.dumps(lines[-1]), flush=True)

    # the corpus form: the trained corpus as ids, window 2
    n_tok = eng.num_tokens()
    eng.export_skipgram_counts_tensors(None, 2, 'ids')   # warm-up
    eng.reset_skipgram_counts_stats()
    got, t_dev = best(lambda: eng.export_skipgram_counts_tensors(None, 2, 'ids'), a.reps)
    torch.cuda.synchronize()
    st = eng.skipgram_counts_stats()
    host, t_host = best(lambda: eng.export_skipgram_counts(None, 2, 'ids'), a.reps)
    pt, pc, _po = eng.export_skipgram(None, 2, 'ids')
    want, t_np = best(lambda: numpy_counts(pt, pc, n_tok), 1)
    res = {'what': 'skip-gram pair counts of corpus samples: the export into scratch, then the counts',
           'workload': 'corpus', 'window': 2, 'dim': n_tok, 'texts': a.texts, 'values': st['values_in'] // a.reps,
           'pairs_counted': st['pairs_counted'] // a.reps, 'distinct': st['distinct_out'] // a.reps,
           'lds_overflow': st['lds_overflow'] // a.reps, 'kernel_ms_per_call': round(st['kernel_ms'] / a.reps, 3),
           'device_with_sizing_ms': round(t_dev * 1e3, 3), 'host_ms': round(t_host * 1e3, 3),
           'numpy_unique_over_pairs_ms': round(t_np * 1e3, 3), 'identical': identical(got, want) and identical(host, want)}
    lines.append(res)
    print(json.dumps(res), flush=True)
    eng.close()
    enc.close()
    if not all(r['identical'] for r in lines):
        sys.exit('a pair-count route and numpy unique over the pairs disagree')
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, 'w') as f:
        f.write('\n'.join(json.dumps(r) for r in lines) + '\n')


if __name__ == '__main__':
    main()
