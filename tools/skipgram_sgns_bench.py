#!/usr/bin/env python3
"""What one negative-sampling step of the skip-gram model costs (csrc/bpe_sgns.hip.h: sgns_adam_step from
device count planes and a shared negative set) beside the full-softmax adam_step on the same planes and
beside the same SGNS step written in torch, all in one run on the same GPU.

The two shapes of tools/skipgram_model_bench.py: the reference's V = 1198, E = 50 on the window-2 counts of
its batch, and V = 16384, E = 64 on synthetic counts (--cells distinct random cells, counts 1..8).  For
each shape and S in --negatives (ids drawn from the noise distribution, weights multiplicity / S, neg_k = 5)
one JSON line, printed and written to profiles/skipgram_sgns_bench.jsonl:
  - the kernels' time per sgns_adam_step (HIP events, bpe_sgmodel_sgns_stats) as the best and the worst of
    --reps warmed steps, the best step's split into transposition, target side and context side, and the
    whole call from device tensors (host clock around the synchronising call);
  - the same for adam_step (the full softmax) on the same planes;
  - the torch step: rows gathered for the U cells, a dense V x S product for the set, logsigmoid, autograd
    and torch.optim.Adam, timed by device events;
  - the first-step loss of the SGNS kernels and of torch.

--form csr | dense | auto is the model's count form (bpe_sgmodel_set_counts_form, both steps) and the records'
`form`; the records of another form than csr are appended to profiles/skipgram_dense_bench.jsonl instead.

Usage: tools/skipgram_sgns_bench.py [--texts 20000] [--reps 10] [--cells 2000000] [--negatives 256 1024] [--form csr]
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
KAPPA = 5.0


def timed_steps(step, stats, reset, reps):
    """(first result, per-step stats, per-step host ms) of one warm-up and `reps` timed calls."""
    first = step()
    per, call_ms = [], []
    for _ in range(reps):
        reset()
        t0 = time.perf_counter()
        step()
        call_ms.append((time.perf_counter() - t0) * 1e3)
        per.append(stats())
    return first, per, call_ms


def measure(name, V, E, planes, S, reps, dev, form='csr'):
    t, c, k = planes
    rng = np.random.default_rng(3)
    a = float(np.sqrt(1.0 / E))
    par = [rng.uniform(-a, a, s).astype(np.float32) for s in ((V, E), (E,), (V, E), (V,))]
    m = pkg.SkipgramModel(0, V, E)
    m.set_counts_form(form)
    q = m.noise(t.cpu().numpy(), c.cpu().numpy(), k.cpu().numpy())
    ids, w = m.sample_negatives(q, S, seed=11)
    d_ids, d_w = torch.from_numpy(ids).to(dev), torch.from_numpy(w).to(dev)

    m.set_params(*par)
    first, per, call_ms = timed_steps(lambda: m.sgns_adam_step_tensors(t, c, k, d_ids, d_w, neg_k=KAPPA, **ADAM),
                                      m.sgns_stats, m.reset_sgns_stats, reps)
    best = min(per, key=lambda s: s['kernel_ms'])
    m.set_params(*par)
    m.reset_optimizer()
    _, full, full_call_ms = timed_steps(lambda: m.adam_step_tensors(t, c, k, **ADAM), m.stats, m.reset_stats, reps)
    m.close()

    # the same SGNS step in torch
    tp = [torch.from_numpy(x).to(dev).requires_grad_() for x in par]
    tl, cl, al, kf = t.long(), c.long(), d_ids.long(), k.float()
    n = torch.zeros(V, dtype=torch.float32, device=dev).index_add_(0, tl, kf)
    P = float(k.sum().item())
    opt = torch.optim.Adam(tp, lr=ADAM['lr'], betas=(ADAM['beta1'], ADAM['beta2']), eps=ADAM['eps'])
    losses, t_ms = [], []

    def torch_step():
        opt.zero_grad(set_to_none=True)
        H = tp[0] + tp[1]
        zp = (H[tl] * tp[2][cl]).sum(1) + tp[3][cl]
        zn = torch.matmul(H, tp[2][al].T) + tp[3][al]
        logsig = torch.nn.functional.logsigmoid
        loss = -((kf * logsig(zp)).sum() + KAPPA * (n[:, None] * d_w[None, :] * logsig(-zn)).sum()) / P
        loss.backward()
        opt.step()
        losses.append(loss)

    for i in range(reps + 1):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        torch_step()
        e1.record()
        torch.cuda.synchronize()
        if i:
            t_ms.append(e0.elapsed_time(e1))
    return {'what': 'skip-gram model: one sgns_adam_step from device count planes, beside adam_step and torch',
            'workload': name, 'form': form, 'V': V, 'E': E, 'U': int(t.numel()), 'P': best['pairs'], 'draws': S,
            'S': int(ids.size), 'neg_k': KAPPA,
            'kernel_ms': round(best['kernel_ms'], 3), 'kernel_ms_worst': round(max(s['kernel_ms'] for s in per), 3),
            'transpose_ms': round(best['transpose_ms'], 3), 'target_ms': round(best['target_ms'], 3),
            'context_ms': round(best['context_ms'], 3),
            'call_ms': round(min(call_ms), 3), 'call_ms_worst': round(max(call_ms), 3),
            'full_softmax_kernel_ms': round(min(s['kernel_ms'] for s in full), 3),
            'full_softmax_kernel_ms_worst': round(max(s['kernel_ms'] for s in full), 3),
            'full_softmax_call_ms': round(min(full_call_ms), 3),
            'torch_sgns_step_ms': round(min(t_ms), 3), 'torch_sgns_step_ms_worst': round(max(t_ms), 3),
            'loss_first_step': first, 'torch_loss_first_step': float(losses[0].item())}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--texts', type=int, default=20000)
    ap.add_argument('--min', type=int, default=16)
    ap.add_argument('--max', type=int, default=1024)
    ap.add_argument('--reps', type=int, default=10)
    ap.add_argument('--merges', type=int, default=100)
    ap.add_argument('--cells', type=int, default=2000000)
    ap.add_argument('--negatives', type=int, nargs='+', default=[256, 1024])
    ap.add_argument('--form', choices=['csr', 'dense', 'auto'], default='csr')
    ap.add_argument('--out')
    a = ap.parse_args()
    a.out = a.out or os.path.join(ROOT, 'profiles', 'skipgram_sgns_bench.jsonl' if a.form == 'csr' else 'skipgram_dense_bench.jsonl')
    if not torch.cuda.is_available():
        sys.exit('skipgram_sgns_bench needs a HIP device')
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
    enc = pkg.Encoder(0, [(m[0], m[1], len(new_chars) + i) for i, m in enumerate(merges)])
    enc.set_chars({int(cp): i for i, cp in enumerate(new_chars)})
    ids, ioff = enc.encode_utf8(data, boff, 'ids')
    eng.close()
    V = 1198   # (the model bench's folding of neighbouring ids into the reference's size)
    vec = np.ascontiguousarray((ids.astype(np.int64) * 197 + np.roll(ids, 1)) % V, np.int32)
    small = enc.skipgram_counts_tensors(torch.from_numpy(vec).to(dev), torch.from_numpy(ioff).to(dev), 2, V)
    enc.close()
    Vb = pkg.SKIPGRAM_COUNTS_MAX_DIM
    keys = torch.unique(torch.randint(0, Vb * Vb, (a.cells,), device=dev, generator=torch.Generator(dev).manual_seed(9)))
    big = ((keys // Vb).int(), (keys % Vb).int(), (keys * 2654435761 % 8 + 1))
    lines = []
    for name, V, E, planes in (('bench_batch_counts', V, 50, small), ('synthetic_counts', Vb, 64, big)):
        for S in a.negatives:
            lines.append(measure(name, V, E, planes, S, a.reps, dev, a.form))
            print(json.dumps(lines[-1]), flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, 'w' if a.form == 'csr' else 'a') as f:
        f.write('\n'.join(json.dumps(r) for r in lines) + '\n')


if __name__ == '__main__':
    main()
