#!/usr/bin/env python3
"""What the line split costs (csrc/bpe_lines.hip.h: texts -> samples on the device, the corpus helpers
linesToCorpus / linesTrimmedToCorpus / fileContentToCorpus) and what add_lines_utf8 takes from host and
from device buffers, against the host route in the same run.

The batch is the text benches' (tools/encode_text_bench.py, tools/utf8_bench.py): a stretch of the
synthetic latin1 stream cut into texts of [min, max] chars, here each text a line, joined by LF into
files of about 1 MiB:
  ascii           every char 0x20 + byte % 95
  cyrillic_cjk    even bytes U+0400 + byte, odd bytes U+4E00 + byte
  ascii_ws_runs   the ascii mix, 1 % of its lines with a run of 1..4096 spaces at their start or end
  single_line     one file that is one line of 2^24 units of the ascii mix, no LF: the same units as
                  one line instead of many (the split must not depend on a line's length)
One JSON line per variant, printed and written to profiles/lines_bench.jsonl: the split's kernel
time (HIP events, mode 'trim', device buffers) as a multiple of a device-to-device copy of the bytes it
reads plus writes (the units once, the kept units again for the emit, the samples written) and as a
share of the 8 TB/s HBM spec peak; units per second; the whole add_lines_utf8 call from host and from
device buffers against the host route (bytes.decode, the helper restated in Python, add_text); and
whether the routes' corpora are identical.

Usage: tools/lines_bench.py [--texts 100000] [--min 16] [--max 1024] [--reps 3]
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

HBM_PEAK_GBS = 8000.0      # MI355X HBM3E spec peak
FILE_UNITS = 1 << 20
VARIANTS = ['ascii', 'cyrillic_cjk', 'ascii_ws_runs', 'single_line']
# what ECMAScript's trim() removes (WhiteSpace and LineTerminator)
JS_WS = ''.join(map(chr, [9, 10, 11, 12, 13, 0x20, 0xA0, 0x1680] + list(range(0x2000, 0x200B)) +
                    [0x2028, 0x2029, 0x202F, 0x205F, 0x3000, 0xFEFF]))


def lines_to_corpus(text):
    return ['\r' + line.strip(JS_WS) + '\n' for line in text.split('\n')]


def render(variant, src, off, rng):
    """The files of the variant, as a list of str."""
    b = src.astype(np.int64)
    cps = np.where(b & 1, 0x4E00 + b, 0x400 + b) if variant == 'cyrillic_cjk' else 0x20 + b % 95
    text = cps.astype('<u4').tobytes().decode('utf-32-le')
    if variant == 'single_line':
        return [text[:1 << 24]]
    lines = [text[off[k]:off[k + 1]] for k in range(len(off) - 1)]
    if variant == 'ascii_ws_runs':
        for k in np.flatnonzero(rng.random(len(lines)) < 0.01):
            run = ' ' * int(rng.integers(1, 4097))
            lines[k] = run + lines[k] if rng.random() < 0.5 else lines[k] + run
    files, cur, n = [], [], 0
    for line in lines:
        cur.append(line)
        n += len(line) + 1
        if n >= FILE_UNITS:
            files.append('\n'.join(cur) + '\n')
            cur, n = [], 0
    if cur:
        files.append('\n'.join(cur))
    return files


def best(fn, reps):
    out, t = None, []
    for _ in range(reps):
        t0 = time.perf_counter()
        out = fn()
        t.append(time.perf_counter() - t0)
    return out, min(t)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--texts', type=int, default=100000)
    ap.add_argument('--min', type=int, default=16)
    ap.add_argument('--max', type=int, default=1024)
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'lines_bench.jsonl'))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit('lines_bench needs a HIP device')
    dev = torch.device('cuda', 0)
    rng = np.random.default_rng(5)
    text_lens = rng.integers(a.min, a.max + 1, size=a.texts)
    src = pkg.synth_latin1(max(int(text_lens.sum()), 1 << 24), seed=12345, A=256, skip=256 << 20)
    off = np.zeros(a.texts + 1, np.int64)
    np.cumsum(text_lens, out=off[1:])
    out_lines = []
    for variant in VARIANTS:
        files = render(variant, src, off, rng)
        raw = [f.encode('utf-8') for f in files]
        data = np.frombuffer(b''.join(raw), np.uint8)
        boff = np.concatenate([[0], np.cumsum([len(r) for r in raw])]).astype(np.int64)
        units = np.frombuffer(''.join(files).encode('utf-16-le'), '<u2').astype(np.uint16)
        uoff = np.concatenate([[0], np.cumsum([len(f) for f in files])]).astype(np.int64)
        d_data, d_boff = torch.from_numpy(data.copy()).to(dev), torch.from_numpy(boff).to(dev)
        d_units, d_uoff = torch.from_numpy(units.view(np.int16).copy()).to(dev), torch.from_numpy(uoff).to(dev)

        # ---- the split alone, device buffers in and out ----
        enc = pkg.Encoder(0)
        enc.split_lines_tensors(d_units, d_uoff, 'trim')   # warm-up
        k_ms = []
        for _ in range(a.reps):
            enc.reset_lines_stats()
            enc.split_lines_tensors(d_units, d_uoff, 'trim')
            st = enc.lines_stats()
            k_ms.append(st['kernel_ms'])
        k_s = min(k_ms) / 1e3
        enc.close()
        kept = st['units_out'] - 2 * st['samples']
        rw = 2 * st['units_in'] + 2 * kept + 2 * st['units_out']
        x = torch.empty(rw, dtype=torch.uint8, device=dev)
        y = torch.empty_like(x)
        c_ms = []
        for _ in range(a.reps + 1):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            y.copy_(x)
            e1.record()
            torch.cuda.synchronize()
            c_ms.append(e0.elapsed_time(e1))
        copy_s = min(c_ms[1:]) / 1e3
        del x, y

        # ---- the ingest: add_lines_utf8 against decode + helper + add_text on the host ----
        def ingest_best(fn, reps):
            ts, corpus = [], None
            for i in range(reps + 1):
                e = pkg.Engine(0)
                t0 = time.perf_counter()
                fn(e)
                ts.append(time.perf_counter() - t0)
                if i == 0:
                    corpus = e.read_corpus()
                e.close()
            return corpus, min(ts[1:])
        strs, t_decode = best(lambda: [r.decode('utf-8', 'replace') for r in raw], 1)
        samples, t_helper = best(lambda: [s for t in strs for s in lines_to_corpus(t)], 1)
        ref, t_add_text = ingest_best(lambda e: e.add_text(samples), 1)
        c, t_host = ingest_best(lambda e: e.add_lines_utf8(data, boff), a.reps)
        same = bool(np.array_equal(c[0], ref[0]) and np.array_equal(c[1], ref[1]))
        c, t_dev = ingest_best(lambda e: e.add_lines_utf8_tensors(d_data, d_boff), a.reps)
        same &= bool(np.array_equal(c[0], ref[0]) and np.array_equal(c[1], ref[1]))

        ms = lambda s: round(s * 1e3, 3)
        res = {
            'what': 'lines as samples: files split into samples on the device in front of the ingest',
            'variant': variant, 'files': len(files), 'bytes': int(data.size), 'units_in': int(st['units_in']),
            'samples': int(st['samples']), 'units_out': int(st['units_out']), 'trimmed': int(st['trimmed']),
            'split_kernel_ms': ms(k_s), 'split_units_per_s': st['units_in'] / k_s,
            'split_read_plus_written_bytes': int(rw), 'split_gbs': rw / k_s / 1e9,
            'split_frac_hbm_peak': rw / k_s / 1e9 / HBM_PEAK_GBS,
            'd2d_copy_of_read_plus_written_ms': ms(copy_s), 'split_over_d2d_copy': k_s / copy_s,
            'add_lines_utf8_host_ms': ms(t_host), 'add_lines_utf8_device_ms': ms(t_dev),
            'host_route_decode_ms': ms(t_decode), 'host_route_helper_ms': ms(t_helper),
            'host_route_add_text_ms': ms(t_add_text), 'host_route_total_ms': ms(t_decode + t_helper + t_add_text),
            'corpora_identical': same,
        }
        print(json.dumps(res), flush=True)
        out_lines.append(json.dumps(res))
        if not same:
            sys.exit('the device route and the host route disagree')
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, 'w') as f:
        f.write('\n'.join(out_lines) + '\n')


if __name__ == '__main__':
    main()
