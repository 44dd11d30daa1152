#!/usr/bin/env python3
"""What the skip-gram model's text calls cost (csrc/bpe_sgtext.hip.h: embed_texts_tensors with pool='mean' and
score_texts_tensors with window 2, from device values and offsets) beside the same results written in torch
(index_select gathers and index_add_ into the texts, in slices of --slice positions so that the gathered rows
fit; the score as gathered dots of the pairs at every distance, minus a logsumexp over the V x V logits), the
two sides alternating in one run on the same GPU.

The two shapes of the model benches (V = 1198, E = 50; V = 16384, E = 64) with seeded random parameters, over
three batches of seeded random values: 100 000 texts of 16..1024 values, one text of 2^24 values, and 2^20
texts of 1..4 values.  For each shape and batch one JSON line, printed and written to
profiles/skipgram_text_bench.jsonl:
  - the kernels' time per call (HIP events: bpe_sgmodel_text_stats; the score's includes its lse forward) and
    the whole call from device tensors (host clock around the synchronising call), each as the best and the
    worst of --reps warmed calls; device events around the torch side;
  - which side was faster, and the largest difference between the two sides' results relative to the largest
    entry.

Usage: tools/skipgram_text_bench.py [--reps 10] [--slice 4194304]
"""
import argparse
import importlib
import json
import os
import sys
import time

import numpy as np

import torch  # (before libbpe loads: PyTorch's HIP runtime must be the process's first)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
pkg = importlib.import_module('bpe-tokenizer_amd')
WINDOW = 2


def torch_pool(X, vals, tid, lens, step):
    out = torch.zeros((lens.numel(), X.shape[1]), dtype=torch.float32, device=X.device)
    for a in range(0, vals.numel(), step):
        out.index_add_(0, tid[a:a + step], X.index_select(0, vals[a:a + step]))
    return out / lens.clamp(min=1).unsqueeze(1).float()


def torch_score(X, Eout, b2, vals, tid, n_texts, step):
    lse = torch.logsumexp(X @ Eout.T + b2, 1)
    out = torch.zeros(n_texts, dtype=torch.float64, device=X.device)
    for a in range(0, vals.numel(), step):
        v, t = vals[a:a + step + WINDOW], tid[a:a + step + WINDOW]   # (the pairs whose first position is in the slice)
        for d in range(1, WINDOW + 1):
            n = min(step, v.numel() - d)
            if n <= 0:
                continue
            keep = t[:n] == t[d:d + n]
            p, q, k = v[:n][keep], v[d:d + n][keep], t[:n][keep]
            for x, y in ((p, q), (q, p)):
                z = (X.index_select(0, x) * Eout.index_select(0, y)).sum(1) + b2.index_select(0, y) - lse.index_select(0, x)
                out.index_add_(0, k, z.double())
    return out


def measure(name, V, E, lens, reps, step, dev):
    g = torch.Generator(dev).manual_seed(11)
    off = torch.zeros(lens.numel() + 1, dtype=torch.int64, device=dev)
    off[1:] = torch.cumsum(lens, 0)
    n_vals = int(off[-1].item())
    vals = torch.randint(0, V, (n_vals,), device=dev, generator=g, dtype=torch.int32)
    vl = vals.long()
    tid = torch.repeat_interleave(torch.arange(lens.numel(), device=dev), lens)
    rng = np.random.default_rng(3)
    a = float(np.sqrt(1.0 / E))
    par = [rng.uniform(-a, a, s).astype(np.float32) for s in ((V, E), (E,), (V, E), (V,))]
    m = pkg.SkipgramModel(0, V, E)
    m.set_params(*par)
    tp = [torch.from_numpy(x).to(dev) for x in par]
    X = tp[0] + tp[1]

    def timed_torch(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        r = fn()
        e1.record()
        torch.cuda.synchronize()
        return r, e0.elapsed_time(e1)

    def timed_ours(fn):
        m.reset_text_stats()
        t0 = time.perf_counter()
        r = fn()
        t1 = time.perf_counter()
        return r, m.text_stats(), (t1 - t0) * 1e3

    ms = {k: [] for k in ('pool_kernel', 'pool_call', 'pool_torch', 'score_kernel', 'score_call', 'score_torch')}
    diff, st = {}, {}
    for i in range(reps + 1):   # (the first round warms both sides up)
        rows, sp, pc = timed_ours(lambda: m.embed_texts_tensors(vals, off, pool='mean'))
        trows, pt = timed_torch(lambda: torch_pool(X, vl, tid, lens, step))
        (sums, pairs), ss, sc = timed_ours(lambda: m.score_texts_tensors(vals, off, window=WINDOW))
        tsums, stt = timed_torch(lambda: torch_score(X, tp[2], tp[3], vl, tid, lens.numel(), step))
        if i == 0:
            diff = {'pool': float(((rows - trows).abs().max() / trows.abs().max()).item()),
                    'score': float(((sums - tsums).abs().max() / tsums.abs().max()).item())}
            st = {'items': sp['items'], 'pairs': ss['pairs']}
            continue
        for k, x in (('pool_kernel', sp['kernel_ms']), ('pool_call', pc), ('pool_torch', pt),
                     ('score_kernel', ss['kernel_ms']), ('score_call', sc), ('score_torch', stt)):
            ms[k].append(x)
    m.close()
    line = {'what': 'skip-gram model over texts: embed_texts_tensors (mean) and score_texts_tensors from device values, '
                    'beside the same results in torch, alternating',
            'workload': name, 'V': V, 'E': E, 'texts': int(lens.numel()), 'values': n_vals, 'items': st['items'],
            'window': WINDOW, 'pairs': st['pairs'], 'text_chunk': pkg.SGM_TEXT_CHUNK, 'reps': reps, 'torch_slice': step}
    for k, x in ms.items():
        line[k + '_ms'] = round(min(x), 3)
        line[k + '_ms_worst'] = round(max(x), 3)
    line['pool_faster'] = 'kernels' if line['pool_call_ms'] < line['pool_torch_ms'] else 'torch'
    line['score_faster'] = 'kernels' if line['score_call_ms'] < line['score_torch_ms'] else 'torch'
    line['pool_max_rel_diff_to_torch'] = '%.3g' % diff['pool']
    line['score_max_rel_diff_to_torch'] = '%.3g' % diff['score']
    line['not_measured'] = ['share of peak', 'weights', 'pool sum / unit', 'other windows', 'E = 256',
                            'more than one run of this tool']
    return line


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=10)
    ap.add_argument('--slice', type=int, default=1 << 22)
    ap.add_argument('--scale', type=float, default=1.0, help='shrinks the batches (a rehearsal)')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'skipgram_text_bench.jsonl'))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit('skipgram_text_bench needs a HIP device')
    dev = torch.device('cuda', 0)
    g = torch.Generator(dev).manual_seed(5)
    n = lambda x: max(1, int(x * a.scale))   # noqa: E731
    batches = [('texts_16_1024', torch.randint(16, 1025, (n(100000),), device=dev, generator=g)),
               ('one_text_2p24', torch.full((1,), n(1 << 24), dtype=torch.int64, device=dev)),
               ('short_texts_1_4', torch.randint(1, 5, (n(1 << 20),), device=dev, generator=g))]
    lines = []
    for V, E in ((1198, 50), (pkg.SKIPGRAM_COUNTS_MAX_DIM, 64)):
        for name, lens in batches:
            lines.append(measure(name, V, E, lens, a.reps, a.slice, dev))
            print(json.dumps(lines[-1]), flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, 'w') as f:
        f.write('\n'.join(json.dumps(r) for r in lines) + '\n')


if __name__ == '__main__':
    main()
