#!/usr/bin/env python3
"""The dense-count form of the skip-gram model's training steps (csrc/bpe_sgdense.hip.h) beside the CSR form
and beside the same step written densely in torch, alternating in one run on the same GPU.

Planes are synthetic: every cell of V x V at density 1, else a random subset, counts 1..8.  Per workload and
mode ('softmax': adam_step, 'sgns': sgns_adam_step with --draws negatives, neg_k = 5) one JSON line, printed
and appended to profiles/skipgram_dense_bench.jsonl: the kernels' time per step (HIP events, the model's
stats, Adam included) of both forms as the best and the worst of --reps warmed steps, torch's step by device
events, the first-step losses of the three, and `dense_wins`: the dense form's best is below the CSR form's
best by more than the CSR form's own best-to-worst spread in this run.
  the shapes   V = 1198, E = 50, all cells (the reference's size) and V = 16384, E = 64, --cells cells;
  --sweep      V = 1198 and 4096, E = 64, densities 1, 1/4, 1/16, 1/64, without torch: the table behind
               BPE_SGM_DENSE_THETA (the smallest density at which dense wins at both sizes in both modes).

Usage: tools/skipgram_dense_bench.py [--reps 10] [--cells 2000000] [--draws 256 1024] [--sweep] [--no-torch]
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
pkg = importlib.import_module('bpe-tokenizer_amd')
ADAM = dict(lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8)
KAPPA = 5.0


def make_planes(V, cells, dev):
    gen = torch.Generator(dev).manual_seed(9)
    if cells >= V * V:
        keys = torch.arange(V * V, device=dev)
    elif V <= 4096:
        keys = torch.randperm(V * V, device=dev, generator=gen)[:cells].sort().values
    else:
        keys = torch.unique(torch.randint(0, V * V, (cells,), device=dev, generator=gen))
    return (keys // V).int(), (keys % V).int(), (keys * 2654435761 % 8 + 1)


def measure(V, E, planes, mode, draws, reps, dev, with_torch):
    t, c, k = planes
    rng = np.random.default_rng(3)
    a = float(np.sqrt(1.0 / E))
    par = [rng.uniform(-a, a, s).astype(np.float32) for s in ((V, E), (E,), (V, E), (V,))]
    models = {form: pkg.SkipgramModel(0, V, E) for form in ('csr', 'dense')}
    neg = ()
    if mode == 'sgns':
        q = np.bincount(c.cpu().numpy(), k.cpu().numpy().astype(np.float64), V) ** 0.75
        ids, w = pkg.SkipgramModel.sample_negatives(q / q.sum(), draws, seed=11)
        neg = (torch.from_numpy(ids).to(dev), torch.from_numpy(w).to(dev))
    for form, m in models.items():
        m.set_params(*par)
        m.set_counts_form(form)

    def step(m):
        m.reset_stats()
        m.reset_sgns_stats()
        if mode == 'sgns':
            loss = m.sgns_adam_step_tensors(t, c, k, *neg, neg_k=KAPPA, **ADAM)
            return loss, m.sgns_stats()['kernel_ms']
        loss = m.adam_step_tensors(t, c, k, **ADAM)
        return loss, m.stats()['kernel_ms']

    torch_step = None
    if with_torch:
        tp = [torch.from_numpy(x).to(dev).requires_grad_() for x in par]
        C = torch.zeros((V, V), dtype=torch.float32, device=dev)
        C[t.long(), c.long()] = k.float()
        P = float(k.sum().item())
        opt = torch.optim.Adam(tp, lr=ADAM['lr'], betas=(ADAM['beta1'], ADAM['beta2']), eps=ADAM['eps'])
        if mode == 'sgns':
            N = C.sum(1)[:, None] * torch.zeros(V, device=dev).index_put_((neg[0].long(),), KAPPA * neg[1])[None, :]

        def torch_step():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            opt.zero_grad(set_to_none=True)
            z = torch.matmul(tp[0] + tp[1], tp[2].T) + tp[3]
            if mode == 'sgns':
                ls = torch.nn.functional.logsigmoid
                loss = -((C * ls(z)).sum() + (N * ls(-z)).sum()) / P
            else:
                loss = -(C * torch.log_softmax(z, dim=1)).sum() / P
            loss.backward()
            opt.step()
            e1.record()
            torch.cuda.synchronize()
            return float(loss.item()), e0.elapsed_time(e1)

    ms = {'csr': [], 'dense': [], 'torch': []}
    first = {}
    for i in range(reps + 1):   # the first round warms all three; the forms and torch alternate
        for name, fn in (('csr', lambda: step(models['csr'])), ('dense', lambda: step(models['dense'])),
                         ('torch', torch_step)):
            if fn is None:
                continue
            loss, x = fn()
            if i:
                ms[name].append(x)
            else:
                first[name] = loss
    splits = models['dense'].dense_stats()['last_splits']
    for m in models.values():
        m.close()
    rec = {'what': 'skip-gram model: one Adam step from device count planes, CSR and dense count forms and torch',
           'mode': mode, 'V': V, 'E': E, 'U': int(t.numel()), 'density': round(t.numel() / V / V, 5),
           'draws': draws if mode == 'sgns' else 0, 'reps': reps, 'dense_splits': splits}
    for name, xs in ms.items():
        if xs:
            rec[name + '_ms'], rec[name + '_ms_worst'] = round(min(xs), 3), round(max(xs), 3)
        if name in first:
            rec[name + '_loss_first_step'] = first[name]
    rec['dense_wins'] = rec['dense_ms'] < rec['csr_ms'] - (rec['csr_ms_worst'] - rec['csr_ms'])
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=10)
    ap.add_argument('--cells', type=int, default=2000000)
    ap.add_argument('--draws', type=int, nargs='+', default=[256, 1024])
    ap.add_argument('--sweep', action='store_true')
    ap.add_argument('--no-torch', action='store_true')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'skipgram_dense_bench.jsonl'))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit('skipgram_dense_bench needs a HIP device')
    dev = torch.device('cuda', 0)
    if a.sweep:
        work = [(V, 64, V * V // d, [a.draws[0]], False) for V in (1198, 4096) for d in (1, 4, 16, 64)]
    else:
        Vb = pkg.SKIPGRAM_COUNTS_MAX_DIM
        work = [(1198, 50, 1198 * 1198, a.draws, not a.no_torch), (Vb, 64, a.cells, a.draws, not a.no_torch)]
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    for V, E, cells, draws, with_torch in work:
        planes = make_planes(V, cells, dev)
        for mode, S in [('softmax', 0)] + [('sgns', s) for s in draws]:
            rec = measure(V, E, planes, mode, S, a.reps, dev, with_torch)
            if a.sweep:
                rec['sweep'] = True
            print(json.dumps(rec), flush=True)
            with open(a.out, 'a') as f:
                f.write(json.dumps(rec) + '\n')


if __name__ == '__main__':
    main()
