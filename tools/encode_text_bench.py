#!/usr/bin/env python3
"""Throughput of the device encoder's text form (bpe_encode_text_batch, csrc/bpe_text.hip.h around
csrc/bpe_encode.hip): encodeToVector (core.ts:392-445) of a batch of UTF-16 texts to vector indices.

The batch is the encoder bench's (tools/encode_bench.py): merges from mergeUntil({min_weight: 2,
max_iterations: M}) on MiB of a synthetic corpus, a later stretch of the same stream cut into texts
of [min, max] chars.  Every base token's char is its latin1 byte; the `supplementary` variant moves
the odd bytes to U+10000 + byte, so about half of a text's chars are surrogate pairs (same ids, same
merges, twice the units for those chars).  Prints one JSON line per variant:
  - the front end's kernel time (HIP events, bpe_encoder_get_text_stats) and units/s, the bytes it
    moves through HBM by its shape (2 B per unit read twice, 4 B per char written, 32 B per text of
    offsets; the char table is L2 reads) and their share of the 8 TB/s spec peak; the merge-rank
    kernels' and the back end's time beside it;
  - units/s of the whole call, host form (copies up, kernels, copies down) and device form (torch
    tensors in and out);
  - baseline: what the id form offers for the same job in the same run — chars to ids on the host
    (vectorised numpy over the units), bpe_encode_batch, a numpy to_vector_index gather — whose
    output must equal the text form's (identical_outputs).

Usage: tools/encode_text_bench.py [--corpus uniform|zipf] [--mib 256] [--merges 8000]
                                  [--texts 100000] [--min 16] [--max 1024] [--reps 5]
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


def host_chars_to_ids(units, off, lut):
    """The host stage the text form replaces: code points of the units (vectorised), then the table."""
    if not ((units & 0xF800) == 0xD800).any():                # no surrogates: a unit is a char
        return lut[units], off
    u = units.astype(np.int64)
    low, high = (u & 0xFC00) == 0xDC00, (u & 0xFC00) == 0xD800
    cont = np.zeros(len(u), bool)
    cont[1:] = low[1:] & high[:-1]
    cont[off[off < len(u)]] = False
    start = ~cont
    nxt = np.zeros(len(u), bool)
    nxt[:-1] = cont[1:]
    lo = np.zeros(len(u), np.int64)
    lo[:-1] = u[1:]
    cp = np.where(nxt, 0x10000 + ((u - 0xD800) << 10) + (lo - 0xDC00), u)[start]
    before = np.concatenate([[0], np.cumsum(start)])
    return lut[cp], before[off]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--corpus', default='uniform')
    ap.add_argument('--mib', type=int, default=256)
    ap.add_argument('--merges', type=int, default=8000)
    ap.add_argument('--texts', type=int, default=100000)
    ap.add_argument('--min', type=int, default=16)
    ap.add_argument('--max', type=int, default=1024)
    ap.add_argument('--reps', type=int, default=5)
    a = ap.parse_args()

    n = a.mib << 20
    rng = np.random.default_rng(5)
    text_lens = rng.integers(a.min, a.max + 1, size=a.texts)
    need = int(text_lens.sum())
    if a.corpus == 'zipf':
        data = pkg.synth_zipf(n + need, seed=12345)
        train, rest = data[:n], data[n:n + need]
    else:
        train = pkg.synth_latin1(n, seed=12345, A=256)
        rest = pkg.synth_latin1(need, seed=12345, A=256, skip=n)
    e = pkg.Engine(0)
    cmap, n_tok, _ = e.add_latin1(train, sample_bytes=1 << 20)
    e.set_mode('incremental')
    got = e.merge_until(0, 2, a.merges)
    e.close()
    merges = np.asarray([(x, y, n_tok + k) for k, (x, y, _w) in enumerate(got)], np.int32)
    rest = rest[cmap[rest] >= 0]
    off = np.zeros(a.texts + 1, np.int64)
    np.cumsum(text_lens, out=off[1:])
    off = np.minimum(off, rest.size)
    seen = np.nonzero(cmap >= 0)[0]
    index = np.arange(n_tok + len(merges), dtype=np.int32)   # every token live: the compact index is 0..n-1
    have_torch = torch is not None and torch.cuda.is_available()

    enc = pkg.Encoder(0, merges)
    variants = ['latin1'] + (['supplementary'] if a.corpus != 'zipf' else [])
    for variant in variants:
        # the char of byte b: U+00bb, or (supplementary, odd b) U+10000 + b
        cp_of = np.arange(256, dtype=np.int64)
        if variant == 'supplementary':
            cp_of[1::2] += 0x10000
        cps = cp_of[rest]
        big = cps > 0xFFFF
        rep = 1 + big
        v = np.repeat(cps - 0x10000, rep)
        second = np.zeros(int(rep.sum()), bool)
        second[np.cumsum(rep) - 1] = big
        units = np.where(second, 0xDC00 + (v & 0x3FF),
                         np.where(np.repeat(big, rep), 0xD800 + (v >> 10), np.repeat(cps, rep))).astype(np.uint16)
        uoff = np.concatenate([[0], np.cumsum(rep)])[off].astype(np.int64)
        enc.set_chars({int(cp_of[b]): int(cmap[b]) for b in seen})
        enc.set_vector_index(index)
        lut = np.full(0x110000, -1, np.int32)
        lut[cp_of[seen]] = cmap[seen]

        vals, voff = enc.encode_text_flat(units, uoff, 'vectors')   # warmup
        enc.reset_stats()
        enc.reset_text_stats()
        t0 = time.perf_counter()
        for _ in range(a.reps):
            vals, voff = enc.encode_text_flat(units, uoff, 'vectors')
        e2e = (time.perf_counter() - t0) / a.reps
        ts, es = enc.text_stats(), enc.stats()
        front = ts['front_ms'] / a.reps / 1e3
        chars = ts['chars'] // a.reps
        dev = None
        if have_torch:
            d = torch.device('cuda', 0)
            d_units, d_off = torch.from_numpy(units.view(np.int16)).to(d), torch.from_numpy(uoff).to(d)
            dv, do = enc.encode_text_tensors(d_units, d_off, 'vectors')
            torch.cuda.synchronize(d)
            t0 = time.perf_counter()
            for _ in range(a.reps):
                dv, do = enc.encode_text_tensors(d_units, d_off, 'vectors')
            torch.cuda.synchronize(d)
            dev = (time.perf_counter() - t0) / a.reps
            dev_same = bool(np.array_equal(dv.cpu().numpy(), vals) and np.array_equal(do.cpu().numpy(), voff))
        # the baseline: host chars -> ids, the id form, a numpy gather
        t_base, t_map = [], []
        for _ in range(max(2, a.reps // 2)):
            t0 = time.perf_counter()
            ids, id_off = host_chars_to_ids(units, uoff, lut)
            t1 = time.perf_counter()
            bo, boff = enc.encode_flat(ids, id_off)
            bvals = index[bo]
            t_base.append(time.perf_counter() - t0)
            t_map.append(t1 - t0)
        base = min(t_base)
        same = bool(np.array_equal(bvals, vals) and np.array_equal(boff, voff))
        hbm = 4 * units.size + 4 * chars + 32 * a.texts
        res = {
            'what': 'encodeToVector of a batch of UTF-16 texts on the device encoder (text form)',
            'variant': variant, 'corpus': a.corpus, 'train_mib': a.mib, 'merges': int(len(merges)),
            'texts': a.texts, 'text_chars': [a.min, a.max], 'units_in': int(units.size), 'chars': int(chars),
            'values_out': int(vals.size),
            'front_ms': front * 1e3, 'front_units_per_s': units.size / front, 'front_hbm_bytes': int(hbm),
            'front_gbs': hbm / front / 1e9, 'front_frac_hbm_peak': hbm / front / 1e9 / HBM_PEAK_GBS,
            'merge_kernel_ms': es['kernel_ms'] / a.reps, 'back_ms': ts['back_ms'] / a.reps,
            'host_form_ms': e2e * 1e3, 'host_form_units_per_s': units.size / e2e,
            'device_form_ms': None if dev is None else dev * 1e3,
            'device_form_units_per_s': None if dev is None else units.size / dev,
            'device_form_identical': None if dev is None else dev_same,
            'baseline': {'kind': 'numpy chars -> ids on the host, bpe_encode_batch, numpy to_vector_index gather',
                         'ms': base * 1e3, 'host_map_ms': min(t_map) * 1e3, 'units_per_s': units.size / base},
            'speedup_host_form': base / e2e, 'speedup_device_form': None if dev is None else base / dev,
            'identical_outputs': same,
        }
        print(json.dumps(res), flush=True)
        if not same:
            sys.exit('the text form and the baseline disagree')
    enc.close()


if __name__ == '__main__':
    main()
