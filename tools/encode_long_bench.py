#!/usr/bin/env python3
"""Long texts through the device encoder, replayed (BPE_LONG_REPLAY, the default) and in segments
(BPE_LONG_SPLIT), in the same run on the same build: csrc/bpe_encode.hip, DESIGN.md §3f.1.

The merges are the encoder bench's (tools/encode_bench.py): mergeUntil({min_weight: 2,
max_iterations: M}) on MiB of the uniform synthetic corpus; the texts are a later, disjoint stretch
of the same stream.  Two shapes: one text of 2^24 chars, and 1000 texts of 2^17 chars.  For each,
the id form (bpe_encode_batch), the text form from host buffers and the text form device to device
(torch tensors) are timed on both routes, the outputs of the two routes must be equal, and one
JSON line per shape goes to stdout and to --out: the times, replay / split, and the split route's
plan (windows, segments, fallbacks, plan_ms beside kernel_ms).

BPE_ENCODE_SPLIT_WINDOW is a build-time constant: to compare windows, build one library per value
(make LIB=... OBJ_DIR=... EXTRA=-DBPE_ENCODE_SPLIT_WINDOW=N), run this tool once per library through
BPE_LIB with --window N, and pass --split-only to the runs after the first (the replay does not
depend on the window).  --merges-file keeps the trained list between such runs.

Usage: tools/encode_long_bench.py [--mib 256] [--merges 8000] [--reps 2] [--window N] [--split-only]
                                  [--merges-file F.npz] [--out profiles/encode_long_bench.jsonl]
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

SHAPES = [('one text of 2^24 chars', 1, 1 << 24), ('1000 texts of 2^17 chars', 1000, 1 << 17)]


def trained(a):
    """(merges, cmap, n_tok): trained here, or read from --merges-file."""
    if a.merges_file and os.path.exists(a.merges_file):
        z = np.load(a.merges_file)
        return z['merges'], z['cmap'], int(z['n_tok'])
    train = pkg.synth_latin1(a.mib << 20, seed=12345, A=256)
    e = pkg.Engine(0)
    cmap, n_tok, _ = e.add_latin1(train, sample_bytes=1 << 20)
    e.set_mode('incremental')
    got = e.merge_until(0, 2, a.merges)
    e.close()
    merges = np.asarray([(x, y, n_tok + k) for k, (x, y, _w) in enumerate(got)], np.int32)
    if a.merges_file:
        np.savez(a.merges_file, merges=merges, cmap=cmap, n_tok=n_tok)
    return merges, cmap, n_tok


def timed(fn, reps):
    fn()                                                      # warmup (tables, scratch engine, staging)
    t0 = time.perf_counter()
    for _ in range(reps):
        out = fn()
    return (time.perf_counter() - t0) / reps * 1e3, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--mib', type=int, default=256)
    ap.add_argument('--merges', type=int, default=8000)
    ap.add_argument('--reps', type=int, default=2)
    ap.add_argument('--window', type=int, default=pkg.ENCODE_SPLIT_WINDOW)
    ap.add_argument('--split-only', action='store_true')
    ap.add_argument('--merges-file')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'encode_long_bench.jsonl'))
    a = ap.parse_args()

    merges, cmap, n_tok = trained(a)
    seen = np.nonzero(cmap >= 0)[0]
    index = np.arange(n_tok + len(merges), dtype=np.int32)   # every token live
    have_torch = torch is not None and torch.cuda.is_available()
    dev = torch.device('cuda', 0) if have_torch else None
    enc = pkg.Encoder(0, merges)
    enc.set_chars({int(b): int(cmap[b]) for b in seen})
    enc.set_vector_index(index)
    modes = ['split'] if a.split_only else ['replay', 'split']
    skip = a.mib << 20
    for what, n_texts, chars in SHAPES:
        rest = pkg.synth_latin1(n_texts * chars, seed=12345, A=256, skip=skip)
        skip += n_texts * chars
        rest = rest[cmap[rest] >= 0]
        off = np.minimum(np.arange(n_texts + 1, dtype=np.int64) * chars, rest.size)
        ids = cmap[rest].astype(np.int32)
        units = rest.astype(np.uint16)
        if have_torch:
            d_units, d_off = torch.from_numpy(units.view(np.int16)).to(dev), torch.from_numpy(off).to(dev)

        def device_form():
            vals, voff = enc.encode_text_tensors(d_units, d_off, 'vectors')
            torch.cuda.synchronize(dev)
            return vals, voff

        res = {'what': what, 'window': a.window, 'train_mib': a.mib, 'merges': int(len(merges)),
               'texts': n_texts, 'text_chars': chars, 'tokens_in': int(ids.size)}
        outs = {}
        for mode in modes:
            enc.set_long_texts(mode)
            r = {}
            enc.reset_stats()
            enc.reset_split_stats()
            r['id_form_ms'], o_ids = timed(lambda: enc.encode_flat(ids, off), a.reps)
            st, ss = enc.stats(), enc.split_stats()
            calls = a.reps + 1
            r['kernel_ms'] = st['kernel_ms'] / calls
            r['texts_replay'] = st['texts_replay'] // calls
            if mode == 'split':
                r.update(plan_ms=ss['plan_ms'] / calls, windows=ss['windows'] // calls,
                         segments=ss['segments'] // calls, texts_split=ss['texts_split'] // calls,
                         texts_fallback=ss['texts_fallback'] // calls)
                if n_texts == 1 and (ids.size - 2) // a.window + 1 != r['windows']:
                    sys.exit('--window %d is not the library\'s (%d windows)' % (a.window, r['windows']))
            r['text_host_form_ms'], o_host = timed(lambda: enc.encode_text_flat(units, off, 'vectors'), a.reps)
            o_dev = None
            if have_torch:
                r['text_device_form_ms'], o_dev = timed(device_form, a.reps)
                o_dev = tuple(x.cpu().numpy() for x in o_dev)
            r['tokens_out'] = int(o_ids[0].size)
            same = np.array_equal(index[o_ids[0]], o_host[0]) and np.array_equal(o_ids[1], o_host[1])
            if o_dev is not None:
                same = same and np.array_equal(o_dev[0], o_host[0]) and np.array_equal(o_dev[1], o_host[1])
            r['forms_identical'] = bool(same)
            outs[mode] = o_ids
            res[mode] = r
        if len(modes) == 2:
            res['identical_outputs'] = bool(np.array_equal(outs['replay'][0], outs['split'][0]) and
                                            np.array_equal(outs['replay'][1], outs['split'][1]))
            for form in ('id_form_ms', 'text_host_form_ms', 'text_device_form_ms'):
                if form in res['split']:
                    res['speedup_' + form[:-3]] = res['replay'][form] / res['split'][form]
        line = json.dumps(res)
        print(line, flush=True)
        with open(a.out, 'a') as f:
            f.write(line + '\n')
        if not all(res[m]['forms_identical'] for m in modes) or not res.get('identical_outputs', True):
            sys.exit('outputs differ')
    enc.close()


if __name__ == '__main__':
    main()
