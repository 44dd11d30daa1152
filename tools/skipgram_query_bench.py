#!/usr/bin/env python3
"""What a query of the skip-gram model costs (csrc/bpe_sgquery.hip.h: the k nearest tokens by cosine and the k
likeliest contexts, device forms) beside the same query written in torch on the same GPU, alternating.

The two shapes of tools/skipgram_model_bench.py (V = 1198, E = 50; V = 16384, E = 64) with random parameters,
n in {1, 1024, V} queries, k = 10.  One JSON line per (shape, n, form), printed and written to
profiles/skipgram_query_bench.jsonl:
  - kernel_ms: the kernels of one call (HIP events, bpe_sgmodel_query_stats), best and worst of --reps warmed calls;
  - call_ms: the whole `_tensors` call by the host clock (it synchronises), best and worst;
  - torch_ms: the comparator by device events, best and worst: torch.topk over X[ids] @ X.T with normalised rows,
    and over log_softmax(H @ Eout.T + b2); it writes the n x V matrix (torch_matrix_bytes) that the kernels do not;
  - product_tflops_over_kernel_time: 2 n V E flop over kernel_ms; splits: the key splits the host chose;
  - ids_agree: the share of the n x k ids that equal the comparator's (near-ties may swap between two fp32 orders).

Usage: tools/skipgram_query_bench.py [--reps 10] [--k 10]
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


def measure(V, E, n, k, form, m, tp, reps, dev):
    ids = torch.randint(0, V, (n,), device=dev, generator=torch.Generator(dev).manual_seed(n)).int()
    Ein, b1, Eout, b2 = tp
    X = Ein + b1
    Xn = X / X.norm(dim=1, keepdim=True)
    lids = ids.long()

    def ours():
        return m.neighbors_tensors(ids, k, 'cosine') if form == 'neighbors' else m.predict_tensors(ids, k)

    def theirs():
        if form == 'neighbors':
            s = Xn[lids] @ Xn.T
            s[torch.arange(n, device=dev), lids] = -float('inf')
            return torch.topk(s, k, dim=1)
        return torch.topk(torch.log_softmax(X[lids] @ Eout.T + b2, dim=1), k, dim=1)

    got, want = ours(), theirs()   # warm-up
    k_ms, call_ms, t_ms = [], [], []
    for _ in range(reps):
        m.reset_query_stats()
        t0 = time.perf_counter()
        ours()
        call_ms.append((time.perf_counter() - t0) * 1e3)
        k_ms.append(m.query_stats()['kernel_ms'])
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        theirs()
        e1.record()
        torch.cuda.synchronize()
        t_ms.append(e0.elapsed_time(e1))
    return {'what': 'skip-gram model query (device form) beside the same query in torch', 'form': form, 'V': V, 'E': E,
            'n': n, 'k': k, 'splits': m.query_stats()['splits'],
            'kernel_ms': round(min(k_ms), 4), 'kernel_ms_worst': round(max(k_ms), 4),
            'call_ms': round(min(call_ms), 4), 'call_ms_worst': round(max(call_ms), 4),
            'torch_ms': round(min(t_ms), 4), 'torch_ms_worst': round(max(t_ms), 4),
            'product_tflops_over_kernel_time': round(2.0 * n * V * E / (min(k_ms) * 1e-3) / 1e12, 4),
            'torch_matrix_bytes': n * V * 4,
            'ids_agree': round(float((got[0].long() == want.indices).float().mean().item()), 6)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=10)
    ap.add_argument('--k', type=int, default=10)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'skipgram_query_bench.jsonl'))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit('skipgram_query_bench needs a HIP device')
    dev = torch.device('cuda', 0)
    lines = []
    for V, E in ((1198, 50), (pkg.SKIPGRAM_COUNTS_MAX_DIM, 64)):
        rng = np.random.default_rng(3)
        s = float(np.sqrt(1.0 / E))
        par = [rng.uniform(-s, s, shape).astype(np.float32) for shape in ((V, E), (E,), (V, E), (V,))]
        m = pkg.SkipgramModel(0, V, E)
        m.set_params(*par)
        tp = [torch.from_numpy(x).to(dev) for x in par]
        for n in (1, 1024, V):
            for form in ('neighbors', 'predict'):
                lines.append(measure(V, E, n, a.k, form, m, tp, a.reps, dev))
                print(json.dumps(lines[-1]), flush=True)
        m.close()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, 'w') as f:
        f.write('\n'.join(json.dumps(r) for r in lines) + '\n')


if __name__ == '__main__':
    main()
