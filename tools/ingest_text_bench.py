#!/usr/bin/env python3
"""Throughput of the corpus ingest from text (bpe_add_text_batch, csrc/bpe_ingest.hip.h): addToCorpus
(core.ts:182-207) of a batch of UTF-16 texts, on the device.

The batch is the text encoder bench's (tools/encode_text_bench.py): a stretch of the synthetic
latin1 stream cut into texts of [min, max] chars, every char U+00bb of its byte; the `supplementary`
variant moves the odd bytes to U+10000 + byte (half the chars are surrogate pairs); `one_char` is the
counters' worst case, every unit the same char.  Every rep ingests into a fresh context, so each
call also discovers and numbers the batch's chars.  One JSON line per variant, printed and appended
to profiles/ingest_text_bench.jsonl:
  - the kernels' time (HIP events, bpe_get_ingest_stats) and units/s, the bytes they move through
    HBM by their shape (2 B per unit read twice, 4 B per char and per separator written) and their
    share of the 8 TB/s spec peak;
  - units/s of the whole call, host form (copy up, kernels, small copies down) and device form
    (torch tensors in);
  - yardstick (a), the host path addToCorpus takes today: chars to ids on the host (vectorised numpy
    over the batch, first-appearance numbering included) plus one add_sample per text, on the first
    --baseline-texts texts; its corpus must equal the text ingest's;
  - yardstick (b), bpe_add_latin1 on the latin1 rendering of the same content (1 B per char read
    where the text ingest reads 2 x 2 B per unit): a factor is expected, not parity.

Usage: tools/ingest_text_bench.py [--texts 100000] [--min 16] [--max 1024] [--reps 5]
                                  [--baseline-texts 20000]
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


def host_ids(units, off):
    """The host stage the text ingest replaces: chars of the units, numbered by first appearance."""
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
    uniq, first, inv = np.unique(cp, return_index=True, return_inverse=True)
    rank = np.empty(len(uniq), np.int32)
    rank[np.argsort(first, kind='stable')] = np.arange(len(uniq), dtype=np.int32)
    before = np.concatenate([[0], np.cumsum(start)])
    return rank[inv], before[off]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--texts', type=int, default=100000)
    ap.add_argument('--min', type=int, default=16)
    ap.add_argument('--max', type=int, default=1024)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--baseline-texts', type=int, default=20000)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'ingest_text_bench.jsonl'))
    a = ap.parse_args()

    rng = np.random.default_rng(5)
    text_lens = rng.integers(a.min, a.max + 1, size=a.texts)
    rest = pkg.synth_latin1(int(text_lens.sum()), seed=12345, A=256, skip=256 << 20)
    off = np.zeros(a.texts + 1, np.int64)
    np.cumsum(text_lens, out=off[1:])
    have_torch = torch is not None and torch.cuda.is_available()
    nb = min(a.baseline_texts, a.texts)
    lines = []
    for variant in ['latin1', 'supplementary', 'one_char']:
        cp_of = np.arange(256, dtype=np.int64)
        if variant == 'supplementary':
            cp_of[1::2] += 0x10000
        src = np.full_like(rest, 0x41) if variant == 'one_char' else rest
        cps = cp_of[src]
        big = cps > 0xFFFF
        rep = 1 + big
        v = np.repeat(cps - 0x10000, rep)
        second = np.zeros(int(rep.sum()), bool)
        second[np.cumsum(rep) - 1] = big
        units = np.where(second, 0xDC00 + (v & 0x3FF),
                         np.where(np.repeat(big, rep), 0xD800 + (v >> 10), np.repeat(cps, rep))).astype(np.uint16)
        uoff = np.concatenate([[0], np.cumsum(rep)])[off].astype(np.int64)

        def fresh_run(fn):
            e = pkg.Engine(0)
            t0 = time.perf_counter()
            out = fn(e)
            dt = time.perf_counter() - t0
            return e, out, dt

        e, _, _ = fresh_run(lambda e: e.add_text_flat(units, uoff))   # warmup
        ids_text, off_text = e.read_corpus()
        e.close()
        kernel, e2e, chars, new_chars = [], [], 0, 0
        for _ in range(a.reps):
            e, _, dt = fresh_run(lambda e: e.add_text_flat(units, uoff))
            st = e.ingest_stats()
            kernel.append(st['kernel_ms'] / 1e3)
            e2e.append(dt)
            chars, new_chars = st['chars'], st['new_chars']
            e.close()
        dev = None
        if have_torch:
            d = torch.device('cuda', 0)
            d_units, d_off = torch.from_numpy(units.view(np.int16)).to(d), torch.from_numpy(uoff).to(d)
            t_dev = []
            for _ in range(a.reps + 1):
                e, _, dt = fresh_run(lambda e: e.add_text_tensors(d_units, d_off))
                t_dev.append(dt)
                e.close()
            dev = min(t_dev[1:])
        # (a) the host path: chars -> ids on the host, one add_sample per text
        boff = uoff[:nb + 1]
        bunits = units[:boff[-1]]
        e = pkg.Engine(0)
        t0 = time.perf_counter()
        ids, id_off = host_ids(bunits, boff)
        t_map = time.perf_counter() - t0
        for i in range(int(ids.max()) + 1 if ids.size else 0):
            e.set_token_len16(i, 1)
        for k in range(nb):
            e.add_sample(ids[id_off[k]:id_off[k + 1]])
        t_a = time.perf_counter() - t0
        ids_a, off_a = e.read_corpus()
        e.close()
        same = bool(np.array_equal(off_a, off_text[:nb + 1]) and np.array_equal(ids_a, ids_text[:off_text[nb]]))
        # (b) bpe_add_latin1 on the latin1 rendering (samples of the mean text length)
        t_b = []
        for _ in range(max(2, a.reps // 2)):
            e, _, dt = fresh_run(lambda e: e.add_latin1(src, sample_bytes=(a.min + a.max) // 2))
            t_b.append(dt)
            e.close()
        k_s, e_s = min(kernel), min(e2e)
        hbm = 4 * units.size + 4 * (chars + a.texts)
        res = {
            'what': 'addToCorpus of a batch of UTF-16 texts on the device (bpe_add_text_batch)',
            'variant': variant, 'texts': a.texts, 'text_chars': [a.min, a.max], 'units': int(units.size),
            'chars': int(chars), 'new_chars': int(new_chars),
            'kernel_ms': k_s * 1e3, 'kernel_units_per_s': units.size / k_s, 'kernel_hbm_bytes': int(hbm),
            'kernel_gbs': hbm / k_s / 1e9, 'kernel_frac_hbm_peak': hbm / k_s / 1e9 / HBM_PEAK_GBS,
            'host_form_ms': e_s * 1e3, 'host_form_units_per_s': units.size / e_s,
            'device_form_ms': None if dev is None else dev * 1e3,
            'device_form_units_per_s': None if dev is None else units.size / dev,
            'baseline_host_path': {'kind': 'numpy chars -> ids for the batch, then add_sample per text',
                                   'texts': nb, 'units': int(bunits.size), 'ms': t_a * 1e3,
                                   'host_map_ms': t_map * 1e3, 'units_per_s': bunits.size / t_a},
            'baseline_add_latin1': {'kind': 'bpe_add_latin1 on the latin1 rendering (1 B per char)',
                                    'bytes': int(src.size), 'ms': min(t_b) * 1e3, 'chars_per_s': src.size / min(t_b)},
            'speedup_vs_host_path': (units.size / e_s) / (bunits.size / t_a),
            'ratio_vs_add_latin1': (chars / e_s) / (src.size / min(t_b)),
            'identical_corpus': same,
        }
        print(json.dumps(res), flush=True)
        lines.append(json.dumps(res))
        if not same:
            sys.exit('the text ingest and the host path disagree')
    with open(a.out, 'w') as f:
        f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
