#!/usr/bin/env python3
"""What the closed-form embeddings of the skip-gram model cost (csrc/bpe_svd.hip.h: ppmi_svd_tensors from device
count planes) beside torch.svd_lowrank(M, q=L, niter=power_iters) on the same PPMI matrix on the same GPU (M
from ppmi_tensors: dense where every cell is present, a sparse COO tensor otherwise), the two alternating in
one run, and how many glove_adam_step calls one ppmi_svd costs.

The two shapes of tools/skipgram_glove_bench.py on synthetic planes (counts 1..8): V = 1198, E = 50 with all
V^2 cells, and V = 16384, E = 64 with --cells distinct random cells; the defaults of ppmi_svd (oversample 16,
four power iterations, the seeded Omega).  For each shape one JSON line, printed and written to
profiles/skipgram_svd_bench.jsonl:
  - the kernels' time per call (HIP events: bpe_sgmodel_svd_stats; device events around svd_lowrank) as the best
    and the worst of --reps warmed calls, the best call's split by kernel (tables and transposition, sparse
    products, Grams, Cholesky, applies, the eigenproblem, signs and store), and the whole call from device
    tensors (host clock around the synchronising call);
  - the kernel time of one glove_adam_step on the same planes, best of --reps, and their ratio;
  - the leading singular values of both.

Usage: tools/skipgram_svd_bench.py [--reps 10] [--cells 2000000]
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
ADAM = dict(lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8)
OVERSAMPLE, POWER_ITERS = 16, 4
KERNELS = ['prep_ms', 'spmm_ms', 'gram_ms', 'chol_ms', 'apply_ms', 'eig_ms', 'finish_ms']


def measure(name, V, E, planes, reps):
    t, c, k = planes
    svd, glove = pkg.SkipgramModel(0, V, E), pkg.SkipgramModel(0, V, E)
    rng = np.random.default_rng(3)
    a = float(np.sqrt(1.0 / E))
    glove.set_params(*[rng.uniform(-a, a, s).astype(np.float32) for s in ((V, E), (E,), (V, E), (V,))])
    L = (E + OVERSAMPLE + 15) // 16 * 16
    m = svd.ppmi_tensors(t, c, k)
    if t.numel() == V * V:
        M = m.reshape(V, V)
    else:
        M = torch.sparse_coo_tensor(torch.stack([t.long(), c.long()]), m, (V, V)).coalesce()

    per = {'svd': [], 'torch': [], 'glove': []}
    call_ms = []
    sig = {}
    for i in range(reps + 1):   # (the first round warms all three up)
        svd.reset_svd_stats()
        t0 = time.perf_counter()
        s_ours = svd.ppmi_svd_tensors(t, c, k, oversample=OVERSAMPLE, power_iters=POWER_ITERS)
        t1 = time.perf_counter()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        _, s_torch, _ = torch.svd_lowrank(M, q=L, niter=POWER_ITERS)
        e1.record()
        torch.cuda.synchronize()
        glove.reset_glove_stats()
        glove.glove_adam_step_tensors(t, c, k, **ADAM)
        if i == 0:
            sig = {'ours': [round(float(x), 4) for x in s_ours[:4]], 'torch': [round(float(x), 4) for x in s_torch[:4].cpu()]}
            continue
        per['svd'].append(svd.svd_stats())
        per['torch'].append(e0.elapsed_time(e1))
        per['glove'].append(glove.glove_stats()['kernel_ms'])
        call_ms.append((t1 - t0) * 1e3)
    best = min(per['svd'], key=lambda s: s['kernel_ms'])
    svd.close()
    glove.close()
    out = {'what': 'skip-gram model: one ppmi_svd from device count planes beside torch.svd_lowrank on the same PPMI '
                   'matrix, alternating, and beside one glove_adam_step',
           'workload': name, 'V': V, 'E': E, 'L': best['L'], 'U': int(t.numel()), 'cells': best['cells'],
           'positive_cells': best['positive_cells'], 'oversample': OVERSAMPLE, 'power_iters': POWER_ITERS, 'reps': reps,
           'dropped_columns': best['dropped_columns'], 'sweeps': best['sweeps'],
           'kernel_ms': round(best['kernel_ms'], 3), 'kernel_ms_worst': round(max(s['kernel_ms'] for s in per['svd']), 3)}
    out.update({p: round(best[p], 3) for p in KERNELS})
    out.update({'call_ms': round(min(call_ms), 3), 'call_ms_worst': round(max(call_ms), 3),
                'torch_svd_lowrank_ms': round(min(per['torch']), 3), 'torch_svd_lowrank_ms_worst': round(max(per['torch']), 3),
                'torch_matrix': 'dense' if t.numel() == V * V else 'sparse_coo',
                'torch_over_ours': round(min(per['torch']) / best['kernel_ms'], 2),
                'glove_adam_step_kernel_ms': round(min(per['glove']), 3),
                'glove_steps_per_svd': round(best['kernel_ms'] / min(per['glove']), 1),
                'sigma_first4': sig['ours'], 'torch_sigma_first4': sig['torch'],
                'not_measured': ['share of peak', 'other oversample or power_iters', 'more than one run of this tool']})
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=10)
    ap.add_argument('--cells', type=int, default=2000000)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'skipgram_svd_bench.jsonl'))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit('skipgram_svd_bench needs a HIP device')
    dev = torch.device('cuda', 0)

    def planes(keys, V):
        return (keys // V).int(), (keys % V).int(), (keys * 2654435761 % 8 + 1)

    Vs, Vb = 1198, pkg.SKIPGRAM_COUNTS_MAX_DIM
    small = planes(torch.arange(Vs * Vs, device=dev), Vs)
    big = planes(torch.unique(torch.randint(0, Vb * Vb, (a.cells,), device=dev, generator=torch.Generator(dev).manual_seed(9))), Vb)
    lines = []
    for name, V, E, p in (('all_cells', Vs, 50, small), ('synthetic_counts', Vb, 64, big)):
        lines.append(measure(name, V, E, p, a.reps))
        print(json.dumps(lines[-1]), flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, 'w') as f:
        f.write('\n'.join(json.dumps(r) for r in lines) + '\n')


if __name__ == '__main__':
    main()
