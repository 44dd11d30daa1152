#!/usr/bin/env python3
"""Throughput of the restore on the device (bpe_restore_text_batch, csrc/bpe_append.hip.h behind the
text encoder): restoreToCorpus (core.ts:213-216) of a batch of UTF-16 texts into a fresh context.

The batches are the other text tools' (tools/encode_text_bench.py, tools/encode_long_bench.py):
merges from mergeUntil({min_weight: 2, max_iterations: M}) on MiB of a synthetic corpus, and a later
stretch of the same stream cut into texts, every char the latin1 char of its byte:
  A  100 000 texts of 16 to 1024 chars, the uniform corpus's merges;
  B  the same shape on the zipf-words corpus and its merges;
  C  1000 texts of 2^17 chars, the uniform merges, long_texts='split'.
For each batch, in one run (one warm-up call, then --reps calls into fresh contexts; min, median
and max are reported), one JSON line printed and written to profiles/restore_text_bench.jsonl:
  (a) the host form, restore_text_flat;
  (b) the device form, restore_text_tensors (torch tensors in);
  (c) what restoreToCorpus does today: Encoder.encode_text per text plus add_sample per text, on the
      first --baseline-texts texts (batch C: --baseline-long texts, with the split encoder); its
      corpus must equal the restore's (identical_corpus);
  (d) encode_text_tensors(kind='ids') alone on the same tensors;
  (e) a device-to-device copy of the appended bytes (4 B per token and per separator);
and the append kernel's time (append_stats) against (e), its bytes by its shape (4 B per token and
8 B per sample read, 4 B per slot written) as a share of the 8 TB/s spec peak, and (b) against (d).

Usage: tools/restore_text_bench.py [--mib 256] [--merges 8000] [--texts 100000] [--reps 5]
                                   [--baseline-texts 20000] [--baseline-long 50] [--batches A,B,C]
"""
import argparse
import importlib
import json
import os
import sys
import time

import numpy as np

try:
    import torch  # noqa: F401  (before libbpe loads: PyTorch's HIP runtime must be the process's first)
except ImportError:
    torch = None

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
pkg = importlib.import_module('bpe-tokenizer_amd')

HBM_PEAK_GBS = 8000.0      # MI355X HBM3E spec peak (MI355X_MICROARCH.md)


def spread(xs):
    xs = sorted(xs)
    return {'min': xs[0] * 1e3, 'median': xs[len(xs) // 2] * 1e3, 'max': xs[-1] * 1e3, 'reps': len(xs)}


def train(corpus, n, need, merges):
    """(char map, char tokens, (a, b, c) merges, the stretch after the training bytes)."""
    if corpus == 'zipf':
        data = pkg.synth_zipf(n + need, seed=12345)
        data, rest = data[:n], data[n:n + need]
    else:
        data = pkg.synth_latin1(n, seed=12345, A=256)
        rest = pkg.synth_latin1(need, seed=12345, A=256, skip=n)
    e = pkg.Engine(0)
    cmap, n_tok, _ = e.add_latin1(data, sample_bytes=1 << 20)
    e.set_mode('incremental')
    got = e.merge_until(0, 2, merges)
    e.close()
    abc = np.asarray([(x, y, n_tok + k) for k, (x, y, _w) in enumerate(got)], np.int32)
    return cmap, n_tok, abc, rest[cmap[rest] >= 0]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--mib', type=int, default=256)
    ap.add_argument('--merges', type=int, default=8000)
    ap.add_argument('--texts', type=int, default=100000)
    ap.add_argument('--min', type=int, default=16)
    ap.add_argument('--max', type=int, default=1024)
    ap.add_argument('--long-texts', type=int, default=1000)
    ap.add_argument('--long-chars', type=int, default=1 << 17)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--baseline-texts', type=int, default=20000)
    ap.add_argument('--baseline-long', type=int, default=50)
    ap.add_argument('--batches', default='A,B,C')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'restore_text_bench.jsonl'))
    a = ap.parse_args()
    if torch is None or not torch.cuda.is_available():
        sys.exit('the device form, (d) and (e) need torch with a HIP device')
    dev = torch.device('cuda', 0)

    n = a.mib << 20
    rng = np.random.default_rng(5)
    text_lens = rng.integers(a.min, a.max + 1, size=a.texts)
    need_short = int(text_lens.sum())
    need_long = a.long_texts * a.long_chars
    trained = {}
    lines = []
    for batch in a.batches.split(','):
        corpus = 'zipf' if batch == 'B' else 'uniform'
        if corpus not in trained:
            trained[corpus] = train(corpus, n, need_short + (need_long if corpus == 'uniform' else 0), a.merges)
        cmap, n_tok, abc, rest = trained[corpus]
        if batch == 'C':
            rest = rest[need_short:]
            off = np.minimum(np.arange(a.long_texts + 1, dtype=np.int64) * a.long_chars, rest.size)
            mode, nb = 'split', min(a.baseline_long, a.long_texts)
        else:
            off = np.zeros(a.texts + 1, np.int64)
            np.cumsum(text_lens, out=off[1:])
            off = np.minimum(off, rest.size)
            mode, nb = 'replay', min(a.baseline_texts, a.texts)
        n_texts = len(off) - 1
        units = rest[:off[-1]].astype(np.uint16)   # (latin1: a char is the unit of its byte)
        enc = pkg.Encoder(0, abc, long_texts=mode)
        enc.set_chars({int(ch): int(cmap[ch]) for ch in range(256) if cmap[ch] >= 0})
        d_units, d_off = torch.from_numpy(units.view(np.int16)).to(dev), torch.from_numpy(off).to(dev)

        def fresh_run(fn):
            e = pkg.Engine(0)
            t0 = time.perf_counter()
            fn(e)
            dt = time.perf_counter() - t0
            return e, dt

        # (a) the host form; the first call is the warm-up, and its corpus is the one compared
        e, _ = fresh_run(lambda e: e.restore_text_flat(enc, units, off))
        ids_restore, off_restore = e.read_corpus()
        e.close()
        t_host, t_kernel = [], []
        for _ in range(a.reps):
            e, dt = fresh_run(lambda e: e.restore_text_flat(enc, units, off))
            t_host.append(dt)
            t_kernel.append(e.append_stats()['kernel_ms'] / 1e3)
            e.close()
        tokens = int(ids_restore.size)
        # (b) the device form
        t_dev = []
        same_dev = True
        for r in range(a.reps + 1):
            e, dt = fresh_run(lambda e: e.restore_text_tensors(enc, d_units, d_off))
            t_dev.append(dt)
            t_kernel.append(e.append_stats()['kernel_ms'] / 1e3)
            if r == 0:
                ids_d, off_d = e.read_corpus()
                same_dev = bool(np.array_equal(ids_d, ids_restore) and np.array_equal(off_d, off_restore))
            e.close()
        t_dev = t_dev[1:]
        # (c) what restoreToCorpus does today: encode_text and add_sample, text by text
        e = pkg.Engine(0)
        one = np.zeros(2, np.int64)
        t0 = time.perf_counter()
        for k in range(nb):
            one[1] = off[k + 1] - off[k]
            vals, _o = enc.encode_text_flat(units[off[k]:off[k + 1]], one, 'ids')
            e.add_sample(vals)
        t_c = time.perf_counter() - t0
        ids_c, off_c = e.read_corpus()
        e.close()
        same = bool(np.array_equal(off_c, off_restore[:nb + 1]) and np.array_equal(ids_c, ids_restore[:off_restore[nb]]))
        # (d) the encoder alone, device form
        t_enc = []
        for _ in range(a.reps + 1):
            t0 = time.perf_counter()
            enc.encode_text_tensors(d_units, d_off, 'ids')
            t_enc.append(time.perf_counter() - t0)
        t_enc = t_enc[1:]
        # (e) a device-to-device copy of the appended bytes
        slots = tokens + n_texts
        src = torch.zeros(slots, dtype=torch.int32, device=dev)
        dst = torch.empty_like(src)
        t_copy = []
        for _ in range(a.reps + 1):
            ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            ev0.record()
            dst.copy_(src)
            ev1.record()
            torch.cuda.synchronize(dev)
            t_copy.append(ev0.elapsed_time(ev1) / 1e3)
        t_copy = t_copy[1:]
        del src, dst
        k_s = min(t_kernel)
        hbm = 4 * tokens + 8 * n_texts + 4 * slots
        res = {
            'what': 'restoreToCorpus of a batch of UTF-16 texts on the device (bpe_restore_text_batch)',
            'batch': batch, 'corpus': corpus, 'train_mib': a.mib, 'merges': int(len(abc)), 'long_texts': mode,
            'texts': n_texts, 'units': int(units.size), 'tokens': tokens,
            'host_form_ms': spread(t_host), 'host_form_units_per_s': units.size / min(t_host),
            'device_form_ms': spread(t_dev), 'device_form_units_per_s': units.size / min(t_dev),
            'device_form_identical_to_host_form': same_dev,
            'baseline_text_by_text': {'kind': 'Encoder.encode_text and add_sample per text (restoreToCorpus today)',
                                      'texts': nb, 'of_texts': n_texts, 'units': int(off[nb] - off[0]),
                                      'ms': t_c * 1e3, 'units_per_s': int(off[nb] - off[0]) / t_c},
            'speedup_vs_text_by_text': (units.size / min(t_dev)) / (int(off[nb] - off[0]) / t_c),
            'encode_alone_device_ms': spread(t_enc),
            'd2d_copy_ms': spread(t_copy), 'd2d_copy_bytes': 4 * slots,
            'append_kernel_ms': spread(t_kernel), 'append_kernel_hbm_bytes': int(hbm),
            'append_kernel_gbs': hbm / k_s / 1e9, 'append_kernel_frac_hbm_peak': hbm / k_s / 1e9 / HBM_PEAK_GBS,
            'append_kernel_over_d2d_copy': k_s / min(t_copy),
            'device_form_minus_encode_alone_ms': (min(t_dev) - min(t_enc)) * 1e3,
            'device_form_over_encode_plus_2_copies': min(t_dev) / (min(t_enc) + 2 * min(t_copy)),
            'identical_corpus': same,
        }
        print(json.dumps(res), flush=True)
        lines.append(json.dumps(res))
        enc.close()
        if not (same and same_dev):
            sys.exit('the restore and the text-by-text path disagree')
    with open(a.out, 'w') as f:
        f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
