#!/usr/bin/env python3
"""What one GloVe step of the skip-gram model costs (csrc/bpe_glove.hip.h: glove_adam_step from device count
planes) beside sgns_adam_step with an empty negative set (the same cells and the same two gathers through
the masked tile loop of csrc/bpe_sgns.hip.h: the baseline) and beside the same GloVe step written in torch
(index_select gathers, autograd, torch.optim.Adam), the three alternating in one run on the same GPU.

The two shapes of tools/skipgram_sgns_bench.py on synthetic planes (counts 1..8): V = 1198, E = 50 with all
V^2 cells, and V = 16384, E = 64 with --cells distinct random cells.  For each shape one JSON line, printed
and written to profiles/skipgram_glove_bench.jsonl:
  - the kernels' time per step (HIP events: bpe_sgmodel_glove_stats / _sgns_stats; device events around the
    torch step) as the best and the worst of --reps warmed steps, the best GloVe step's split into
    transposition, target side and context side, and the whole call from device tensors (host clock around
    the synchronising call);
  - the first-step losses of the GloVe kernels and of torch.

Usage: tools/skipgram_glove_bench.py [--reps 10] [--cells 2000000]
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
X_MAX, ALPHA = 100.0, 0.75


def measure(name, V, E, planes, reps, dev):
    t, c, k = planes
    rng = np.random.default_rng(3)
    a = float(np.sqrt(1.0 / E))
    par = [rng.uniform(-a, a, s).astype(np.float32) for s in ((V, E), (E,), (V, E), (V,), (V,))]
    glove, sgns = pkg.SkipgramModel(0, V, E), pkg.SkipgramModel(0, V, E)
    for m in (glove, sgns):
        m.set_params(*par[:4])
    glove.set_target_bias(par[4])
    none = torch.empty(0, dtype=torch.int32, device=dev)

    tp = [torch.from_numpy(x).to(dev).requires_grad_() for x in par]
    tl, cl = t.long(), c.long()
    ell = torch.log(k.double()).float()
    f = torch.clamp((k.double() / X_MAX) ** ALPHA, max=1.0).float()
    opt = torch.optim.Adam(tp, lr=ADAM['lr'], betas=(ADAM['beta1'], ADAM['beta2']), eps=ADAM['eps'])

    def torch_step():
        opt.zero_grad(set_to_none=True)
        H = tp[0] + tp[1]
        z = (H.index_select(0, tl) * tp[2].index_select(0, cl)).sum(1) + tp[3].index_select(0, cl) + tp[4].index_select(0, tl)
        loss = (f * (z - ell) ** 2).sum() / (2 * t.numel())
        loss.backward()
        opt.step()
        return loss

    per = {'glove': [], 'sgns': [], 'torch': []}
    call_ms = {'glove': [], 'sgns': []}
    first = {}
    for i in range(reps + 1):   # (the first round warms all three up)
        glove.reset_glove_stats()
        t0 = time.perf_counter()
        lg = glove.glove_adam_step_tensors(t, c, k, x_max=X_MAX, alpha=ALPHA, **ADAM)
        t1 = time.perf_counter()
        sgns.reset_sgns_stats()
        t2 = time.perf_counter()
        sgns.sgns_adam_step_tensors(t, c, k, none, None, neg_k=0.0, **ADAM)
        t3 = time.perf_counter()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        lt = torch_step()
        e1.record()
        torch.cuda.synchronize()
        if i == 0:
            first = {'glove': lg, 'torch': float(lt.item())}
            continue
        per['glove'].append(glove.glove_stats())
        per['sgns'].append(sgns.sgns_stats()['kernel_ms'])
        per['torch'].append(e0.elapsed_time(e1))
        call_ms['glove'].append((t1 - t0) * 1e3)
        call_ms['sgns'].append((t3 - t2) * 1e3)
    best = min(per['glove'], key=lambda s: s['kernel_ms'])
    glove.close()
    sgns.close()
    return {'what': 'skip-gram model: one glove_adam_step from device count planes, beside sgns_adam_step with an empty '
                    'negative set and torch, alternating',
            'workload': name, 'V': V, 'E': E, 'U': int(t.numel()), 'cells': best['cells'], 'runs': best['runs'],
            'glove_run': pkg.GLOVE_RUN, 'x_max': X_MAX, 'alpha': ALPHA, 'reps': reps,
            'kernel_ms': round(best['kernel_ms'], 3), 'kernel_ms_worst': round(max(s['kernel_ms'] for s in per['glove']), 3),
            'transpose_ms': round(best['transpose_ms'], 3), 'target_ms': round(best['target_ms'], 3),
            'context_ms': round(best['context_ms'], 3),
            'call_ms': round(min(call_ms['glove']), 3), 'call_ms_worst': round(max(call_ms['glove']), 3),
            'sgns_empty_kernel_ms': round(min(per['sgns']), 3), 'sgns_empty_kernel_ms_worst': round(max(per['sgns']), 3),
            'sgns_empty_call_ms': round(min(call_ms['sgns']), 3), 'sgns_empty_call_ms_worst': round(max(call_ms['sgns']), 3),
            'torch_glove_step_ms': round(min(per['torch']), 3), 'torch_glove_step_ms_worst': round(max(per['torch']), 3),
            'loss_first_step': '%.8g' % first['glove'], 'torch_loss_first_step': '%.8g' % first['torch'],
            'not_measured': ['share of peak', 'E = 256', 'more than one run of this tool']}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=10)
    ap.add_argument('--cells', type=int, default=2000000)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'skipgram_glove_bench.jsonl'))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit('skipgram_glove_bench needs a HIP device')
    dev = torch.device('cuda', 0)

    def planes(keys, V):
        return (keys // V).int(), (keys % V).int(), (keys * 2654435761 % 8 + 1)

    Vs, Vb = 1198, pkg.SKIPGRAM_COUNTS_MAX_DIM
    small = planes(torch.arange(Vs * Vs, device=dev), Vs)
    big = planes(torch.unique(torch.randint(0, Vb * Vb, (a.cells,), device=dev, generator=torch.Generator(dev).manual_seed(9))), Vb)
    lines = []
    for name, V, E, p in (('all_cells', Vs, 50, small), ('synthetic_counts', Vb, 64, big)):
        lines.append(measure(name, V, E, p, a.reps, dev))
        print(json.dumps(lines[-1]), flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, 'w') as f:
        f.write('\n'.join(json.dumps(r) for r in lines) + '\n')


if __name__ == '__main__':
    main()
