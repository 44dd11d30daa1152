#!/usr/bin/env python3
"""What one step of the skip-gram model costs (csrc/bpe_sgmodel.hip: loss, gradients and Adam from the
count planes on the device) beside the same step written densely in torch on the same GPU.

Two shapes: the reference's V = 1198, E = 50 on the window-2 counts of tools/skipgram_counts_bench.py's
batch (its encoder output as vectors, folded into V), and V = 16384, E = 64 on synthetic counts (--cells
distinct random cells, counts 1..8).  One JSON line per shape, printed and written to
profiles/skipgram_model_bench.jsonl:
  - U and P; the kernels' time per adam_step (HIP events, bpe_sgmodel_stats) as the best and the worst of
    --reps steps, and the whole adam_step call from device planes (host clock around the synchronising call);
  - the fp32 rate of the four V x V x E products the step makes (S twice, O, dEout: 8 V^2 E flop) over the
    kernels' time, and torch's fp32 `matmul` rate for H @ Eout^T at the same shape as the yardstick;
  - the dense torch step in the same run: C as a V x V fp32 matrix, `matmul`, `log_softmax`, autograd and
    torch.optim.Adam, timed by device events, and its loss beside the model's.

--form csr | dense | auto is the model's count form (bpe_sgmodel_set_counts_form) and the records' `form`; the
records of another form than csr are appended to profiles/skipgram_dense_bench.jsonl instead.

Usage: tools/skipgram_model_bench.py [--texts 20000] [--reps 10] [--cells 2000000] [--form csr]
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


def event_ms(fn, reps):
    """Device-event times of `reps` calls of fn, after one warm-up."""
    fn()
    out = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1))
    return out


def measure(name, V, E, planes, reps, dev, form='csr'):
    t, c, k = planes
    rng = np.random.default_rng(3)
    a = float(np.sqrt(1.0 / E))
    par = [rng.uniform(-a, a, s).astype(np.float32) for s in ((V, E), (E,), (V, E), (V,))]
    m = pkg.SkipgramModel(0, V, E)
    m.set_counts_form(form)
    m.set_params(*par)
    first = m.adam_step_tensors(t, c, k, **ADAM)   # warm-up
    k_ms, call_ms = [], []
    for _ in range(reps):
        m.reset_stats()
        t0 = time.perf_counter()
        m.adam_step_tensors(t, c, k, **ADAM)
        call_ms.append((time.perf_counter() - t0) * 1e3)
        k_ms.append(m.stats()['kernel_ms'])
    st = m.stats()
    m.close()

    # the same step, dense, in torch
    tp = [torch.from_numpy(x).to(dev).requires_grad_() for x in par]
    C = torch.zeros((V, V), dtype=torch.float32, device=dev)
    C[t.long(), c.long()] = k.float()
    P = float(k.sum().item())
    opt = torch.optim.Adam(tp, lr=ADAM['lr'], betas=(ADAM['beta1'], ADAM['beta2']), eps=ADAM['eps'])
    losses = []

    def dense_step():
        opt.zero_grad(set_to_none=True)
        z = torch.matmul(tp[0] + tp[1], tp[2].T) + tp[3]
        loss = -(C * torch.log_softmax(z, dim=1)).sum() / P
        loss.backward()
        opt.step()
        losses.append(loss)

    d_ms = event_ms(dense_step, reps)
    with torch.no_grad():
        H, Eo = tp[0] + tp[1], tp[2]
        mm_ms = event_ms(lambda: torch.matmul(H, Eo.T), reps)
    flop = 2.0 * V * V * E
    return {'what': 'skip-gram model: one adam_step from device count planes, beside the dense torch step',
            'workload': name, 'form': form, 'V': V, 'E': E, 'U': int(t.numel()), 'P': st['pairs'],
            'kernel_ms': round(min(k_ms), 3), 'kernel_ms_worst': round(max(k_ms), 3),
            'adam_step_call_ms': round(min(call_ms), 3), 'adam_step_call_ms_worst': round(max(call_ms), 3),
            'products_tflops_over_kernel_time': round(4 * flop / (min(k_ms) * 1e-3) / 1e12, 3),
            'torch_dense_step_ms': round(min(d_ms), 3), 'torch_dense_step_ms_worst': round(max(d_ms), 3),
            'torch_matmul_ms': round(min(mm_ms), 4), 'torch_matmul_tflops': round(flop / (min(mm_ms) * 1e-3) / 1e12, 3),
            'loss_first_step': first, 'torch_loss_first_step': float(losses[0].item())}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--texts', type=int, default=20000)
    ap.add_argument('--min', type=int, default=16)
    ap.add_argument('--max', type=int, default=1024)
    ap.add_argument('--reps', type=int, default=10)
    ap.add_argument('--merges', type=int, default=100)
    ap.add_argument('--cells', type=int, default=2000000)
    ap.add_argument('--form', choices=['csr', 'dense', 'auto'], default='csr')
    ap.add_argument('--out')
    a = ap.parse_args()
    a.out = a.out or os.path.join(ROOT, 'profiles', 'skipgram_model_bench.jsonl' if a.form == 'csr' else 'skipgram_dense_bench.jsonl')
    if not torch.cuda.is_available():
        sys.exit('skipgram_model_bench needs a HIP device')
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
    # vectors of the reference's size: pairs of neighbouring ids folded into V values, so that the counts
    # fill a V x V matrix the way a vocabulary of V tokens would
    V = 1198
    vec = np.ascontiguousarray((ids.astype(np.int64) * 197 + np.roll(ids, 1)) % V, np.int32)
    planes = enc.skipgram_counts_tensors(torch.from_numpy(vec).to(dev), torch.from_numpy(ioff).to(dev), 2, V)
    enc.close()
    lines = [measure('bench_batch_counts', V, 50, planes, a.reps, dev, a.form)]
    print(json.dumps(lines[-1]), flush=True)

    V = pkg.SKIPGRAM_COUNTS_MAX_DIM
    keys = torch.unique(torch.randint(0, V * V, (a.cells,), device=dev, generator=torch.Generator(dev).manual_seed(9)))
    planes = ((keys // V).int(), (keys % V).int(), (keys * 2654435761 % 8 + 1))
    lines.append(measure('synthetic_counts', V, 64, planes, a.reps, dev, a.form))
    print(json.dumps(lines[-1]), flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, 'w' if a.form == 'csr' else 'a') as f:
        f.write('\n'.join(json.dumps(r) for r in lines) + '\n')


if __name__ == '__main__':
    main()
