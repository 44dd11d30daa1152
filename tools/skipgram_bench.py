#!/usr/bin/env python3
"""What the skip-gram expansion costs (csrc/bpe_skipgram.hip.h: values -> (target, context) planes on
the device) and what the forms built on it take, from host and from device buffers.

The batch is tools/utf8_out_bench.py's ascii one: a stretch of the synthetic latin1 stream cut into
texts of [min, max] chars, ingested, trained for --merges merges, and encoded to ids by the encoder;
what is expanded is that encoder output, and for the corpus form that trained corpus.
One JSON line per workload, printed and written to profiles/skipgram_bench.jsonl:
  - encoder_output, window 2 and 5; one_text of 2^24 values, window 2; corpus, window 2;
  - the two kernels' time (HIP events, bpe_skipgram_stats, device buffers in and out), its ratio to a
    device-to-device copy (torch, CUDA events) of the bytes it reads plus writes (4 B per value and
    8 B per text read, 8 B per pair and 8 B per text written), and its share of the 8 TB/s HBM spec
    peak by those bytes;
  - the whole call from host buffers (the flat form: sizing call, then the pairs) and from device
    buffers (torch tensors, into preallocated planes and with the sizing call);
  - for comparison, in the same run, a vectorised numpy expansion on the host (texts in groups, one
    row of offsets per value) and whether its output was identical.

Usage: tools/skipgram_bench.py [--texts 100000] [--min 16] [--max 1024] [--reps 3] [--merges 100]
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
from utf8_bench import HBM_PEAK_GBS, best  # noqa: E402
from utf8_out_bench import d2d_copy_s  # noqa: E402


def numpy_expand(vals, off, w, group=1 << 20):
    """The pairs of a flat batch on the host: whole texts in groups of about `group` values; per group
    a row of the 2w + 1 places around every value, struck out where they leave the text or are the
    value itself, read row by row."""
    n = len(off) - 1
    ts, cs = [], []
    k = 0
    while k < n:
        k1 = int(np.searchsorted(off, off[k] + group, side='right'))
        k1 = min(max(k1 - 1, k + 1), n)
        a, b = int(off[k]), int(off[k1])
        v = vals[a:b]
        start = np.repeat(off[k:k1] - a, np.diff(off[k:k1 + 1]))
        end = np.repeat(off[k + 1:k1 + 1] - a, np.diff(off[k:k1 + 1]))
        i = np.arange(b - a)[:, None]
        j = i + np.arange(-w, w + 1)[None, :]
        keep = (j >= start[:, None]) & (j != i) & (j < end[:, None])
        ts.append(np.broadcast_to(v[:, None], j.shape)[keep])
        cs.append(v[np.clip(j, 0, max(b - a - 1, 0))][keep])
        k = k1
    return np.concatenate(ts) if ts else vals[:0], np.concatenate(cs) if cs else vals[:0]


def measure(name, enc, vals, off, w, reps, dev, host_compare=True):
    d_vals, d_off = torch.from_numpy(vals).to(dev), torch.from_numpy(off).to(dev)
    t, c, po = enc.skipgram_tensors(d_vals, d_off, w)   # warm-up; sizes the planes
    n_pairs = int(t.numel())
    planes = (torch.empty_like(t), torch.empty_like(c))
    k_ms = []
    for _ in range(reps):
        enc.reset_skipgram_stats()
        enc.skipgram_tensors(d_vals, d_off, w, out=planes)
        k_ms.append(enc.skipgram_stats()['kernel_ms'])
    k_s = min(k_ms) / 1e3
    moved = 4 * len(vals) + 8 * len(off) + 8 * n_pairs + 8 * len(off)
    copy_s = d2d_copy_s(moved, reps, dev)
    _, t_dev_out = best(lambda: enc.skipgram_tensors(d_vals, d_off, w, out=planes), reps + 1)
    _, t_dev = best(lambda: enc.skipgram_tensors(d_vals, d_off, w), reps + 1)
    host, t_host = best(lambda: enc.skipgram_flat(vals, off, w), reps)
    same_forms = bool(np.array_equal(host[0], planes[0].cpu().numpy()) and np.array_equal(host[1], planes[1].cpu().numpy())
                      and np.array_equal(host[2], po.cpu().numpy()))
    res = {'what': 'skip-gram pairs: values expanded into (target, context) planes on the device',
           'workload': name, 'window': w, 'texts': len(off) - 1, 'values': int(len(vals)), 'pairs': n_pairs,
           'kernel_ms': round(k_s * 1e3, 3), 'pairs_per_s': n_pairs / k_s, 'hbm_bytes': int(moved),
           'gbs': moved / k_s / 1e9, 'frac_hbm_peak': moved / k_s / 1e9 / HBM_PEAK_GBS,
           'd2d_copy_of_read_plus_written_ms': round(copy_s * 1e3, 3), 'kernel_over_d2d_copy': k_s / copy_s,
           'device_into_planes_ms': round(t_dev_out * 1e3, 3), 'device_with_sizing_ms': round(t_dev * 1e3, 3),
           'host_ms': round(t_host * 1e3, 3), 'host_form_identical_to_device_form': same_forms}
    if host_compare:
        want, t_np = best(lambda: numpy_expand(vals, off, w), 1)
        res['numpy_host_ms'] = round(t_np * 1e3, 3)
        res['identical_to_numpy'] = bool(np.array_equal(want[0], host[0]) and np.array_equal(want[1], host[1]))
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--texts', type=int, default=100000)
    ap.add_argument('--min', type=int, default=16)
    ap.add_argument('--max', type=int, default=1024)
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--merges', type=int, default=100)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'skipgram_bench.jsonl'))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit('skipgram_bench needs a HIP device')
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
    ids = np.ascontiguousarray(ids)

    lines = []
    for w in (2, 5):
        lines.append(measure('encoder_output', enc, ids, ioff, w, a.reps, dev))
        print(json.dumps(lines[-1]), flush=True)
    one = (np.arange(1 << 24, dtype=np.int64) * 2654435761 % 50021).astype(np.int32)
    lines.append(measure('one_text', enc, one, np.asarray([0, 1 << 24], np.int64), 2, a.reps, dev))
    print(json.dumps(lines[-1]), flush=True)

    # the corpus form: the trained corpus (the batch's texts, merged) as ids, window 2
    vals, voff = eng.export_samples()
    want = numpy_expand(np.ascontiguousarray(vals), voff, 2)
    eng.export_skipgram_tensors(None, 2, 'ids')          # warm-up
    eng.reset_skipgram_stats()
    eng.reset_export_stats()
    got, t_dev = best(lambda: eng.export_skipgram_tensors(None, 2, 'ids'), a.reps)
    torch.cuda.synchronize()
    st, xst = eng.skipgram_stats(), eng.export_stats()
    host, t_host = best(lambda: eng.export_skipgram(None, 2, 'ids'), a.reps)
    n_pairs = int(got[0].numel())
    # (each wrapper call is a sizing call and the real one: the export runs in both, the expand kernel in one)
    res = {'what': 'skip-gram pairs of corpus samples: the export into scratch, then the expansion',
           'workload': 'corpus', 'window': 2, 'texts': len(voff) - 1, 'values': int(len(vals)), 'pairs': n_pairs,
           'skipgram_kernel_ms_per_call': round(st['kernel_ms'] / a.reps, 3),
           'export_kernel_ms_per_call': round(xst['kernel_ms'] / a.reps, 3),
           'device_with_sizing_ms': round(t_dev * 1e3, 3), 'host_ms': round(t_host * 1e3, 3),
           'identical_to_numpy': bool(np.array_equal(want[0], host[0]) and np.array_equal(want[1], host[1])
                                      and np.array_equal(want[0], got[0].cpu().numpy())
                                      and np.array_equal(want[1], got[1].cpu().numpy()))}
    lines.append(res)
    print(json.dumps(res), flush=True)
    eng.close()
    enc.close()
    if not all(r.get('identical_to_numpy', True) and r.get('host_form_identical_to_device_form', True) for r in lines):
        sys.exit('a skip-gram route and the numpy expansion disagree')
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, 'w') as f:
        f.write('\n'.join(json.dumps(r) for r in lines) + '\n')


if __name__ == '__main__':
    main()
