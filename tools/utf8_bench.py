#!/usr/bin/env python3
"""What the UTF-8 front costs (csrc/bpe_utf8.hip.h: bytes -> UTF-16 units on the device) and what the
three pipelines built on it take, from host and from device buffers.

The batch is the text benches' (tools/encode_text_bench.py, tools/ingest_text_bench.py): a stretch of
the synthetic latin1 stream cut into texts of [min, max] chars, rendered as UTF-8 in four mixes:
  ascii           every char 0x20 + byte % 95
  cyrillic_cjk    even bytes U+0400 + byte, odd bytes U+4E00 + byte (2- and 3-byte sequences)
  half_supp       even bytes ASCII, odd bytes U+10000 + byte (4-byte sequences, surrogate pairs)
  ascii_1pct_bad  the ascii mix with 1 % of its bytes replaced by random bytes (ill-formed input)
One JSON line per mix, printed and written to profiles/utf8_bench.jsonl:
  - the transcode's kernel time (HIP events, bpe_utf8_stats, device buffers in and out), its ratio
    to a device-to-device copy of as many bytes as it reads plus writes (torch, CUDA events), and its
    share of the 8 TB/s HBM spec peak by its own bytes: 2 reads of each input byte + 2 B per unit;
  - the whole add_utf8_batch, encode_utf8 and restore_utf8_batch calls from host buffers (the flat
    form) and from device buffers (torch tensors);
  - for comparison, in the same run, what a caller does today: bytes.decode('utf-8', 'replace') per
    text on the host, then the UTF-16 form on the strings (add_text, encode_text, restore_text, which
    encode each string as utf-16-le); and the UTF-16 host form on units prepared beforehand
    (add_text_flat and the like: the copies and kernels alone);
  - whether each route's output was identical to the UTF-16 form's.
The encoder holds the chars of the batch and the first --merges merges trained on it.

Usage: tools/utf8_bench.py [--texts 100000] [--min 16] [--max 1024] [--reps 3] [--merges 100]
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

HBM_PEAK_GBS = 8000.0      # MI355X HBM3E spec peak (MI355X_MICROARCH.md)
MIXES = ['ascii', 'cyrillic_cjk', 'half_supp', 'ascii_1pct_bad']


def render(mix, src, off, rng):
    """(uint8 bytes, int64 byte offsets) of the texts src[off[k]:off[k+1]] in the mix."""
    b = src.astype(np.int64)
    if mix in ('ascii', 'ascii_1pct_bad'):
        cps = 0x20 + b % 95
    elif mix == 'cyrillic_cjk':
        cps = np.where(b & 1, 0x4E00 + b, 0x400 + b)
    else:
        cps = np.where(b & 1, 0x10000 + b, 0x20 + b % 95)
    width = 1 + (cps > 0x7F) + (cps > 0x7FF) + (cps > 0xFFFF)
    boff = np.concatenate([[0], np.cumsum(width)])[off].astype(np.int64)
    data = np.frombuffer(cps.astype('<u4').tobytes().decode('utf-32-le').encode('utf-8'), np.uint8)
    if mix == 'ascii_1pct_bad':
        data = data.copy()
        hit = rng.random(data.size) < 0.01
        data[hit] = rng.integers(0, 256, int(hit.sum()), dtype=np.uint8)
    assert data.size == boff[-1]
    return data, boff


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
    ap.add_argument('--merges', type=int, default=100)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'utf8_bench.jsonl'))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit('utf8_bench needs a HIP device')
    dev = torch.device('cuda', 0)
    rng = np.random.default_rng(5)
    text_lens = rng.integers(a.min, a.max + 1, size=a.texts)
    src = pkg.synth_latin1(int(text_lens.sum()), seed=12345, A=256, skip=256 << 20)
    off = np.zeros(a.texts + 1, np.int64)
    np.cumsum(text_lens, out=off[1:])
    lines = []
    for mix in MIXES:
        data, boff = render(mix, src, off, rng)
        blob = data.tobytes()
        texts = [blob[boff[k]:boff[k + 1]] for k in range(a.texts)]
        d_data, d_off = torch.from_numpy(data.copy()).to(dev), torch.from_numpy(boff).to(dev)

        # what a caller does today: decode on the host, then the UTF-16 form
        strs, t_decode = best(lambda: [t.decode('utf-8', 'replace') for t in texts], 1)
        units = np.frombuffer(''.join(strs).encode('utf-16-le', 'surrogatepass'), '<u2').astype(np.uint16)
        uoff = np.concatenate([[0], np.cumsum([len(s.encode('utf-16-le', 'surrogatepass')) // 2 for s in strs])]).astype(np.int64)

        # ---- the transcode alone, device buffers in and out ----
        enc = pkg.Encoder(0)
        d_units, d_uoff = enc.utf8_to_utf16_tensors(d_data, d_off)   # warm-up
        same_units = bool(np.array_equal(d_units.cpu().numpy().view(np.uint16), units) and
                          np.array_equal(d_uoff.cpu().numpy(), uoff))
        k_ms = []
        for _ in range(a.reps):
            enc.reset_utf8_stats()
            enc.utf8_to_utf16_tensors(d_data, d_off)
            st = enc.utf8_stats()
            k_ms.append(st['kernel_ms'])
        k_s = min(k_ms) / 1e3
        moved = 2 * data.size + 2 * units.size          # 2 reads of each byte + 2 B per unit
        rw = data.size + 2 * units.size                 # bytes it reads plus writes, once each
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

        # ---- the ingest ----
        def ingest(fn):
            e = pkg.Engine(0)
            t0 = time.perf_counter()
            fn(e)
            dt = time.perf_counter() - t0
            return e, dt

        def ingest_best(fn):
            ts, corpus = [], None
            for i in range(a.reps + 1):
                e, dt = ingest(fn)
                ts.append(dt)
                if i == 0:
                    corpus = e.read_corpus()
                e.close()
            return corpus, min(ts[1:])
        ref_corpus, t_add16 = ingest_best(lambda e: e.add_text_flat(units, uoff))
        c, t_add8 = ingest_best(lambda e: e.add_utf8_batch(data, boff))
        same_add = bool(np.array_equal(c[0], ref_corpus[0]) and np.array_equal(c[1], ref_corpus[1]))
        c, t_add8_dev = ingest_best(lambda e: e.add_utf8_tensors(d_data, d_off))
        same_add &= bool(np.array_equal(c[0], ref_corpus[0]) and np.array_equal(c[1], ref_corpus[1]))
        _, t_add_today = ingest_best(lambda e: e.add_text(strs))

        # ---- the encoder: the batch's chars and the first merges trained on it ----
        e = pkg.Engine(0)
        new_chars, _ = e.add_utf8_batch(data, boff)
        merges = e.merge_until(0, 2, a.merges)
        e.close()
        n_chars = len(new_chars)
        enc.add_merges([(m[0], m[1], n_chars + i) for i, m in enumerate(merges)])
        enc.set_chars({int(cp): i for i, cp in enumerate(new_chars)})
        ref_vals, t_enc16 = best(lambda: enc.encode_text_flat(units, uoff, 'ids'), a.reps + 1)
        v, t_enc8 = best(lambda: enc.encode_utf8(data, boff, 'ids'), a.reps + 1)
        same_enc = bool(np.array_equal(v[0], ref_vals[0]) and np.array_equal(v[1], ref_vals[1]))
        v, t_enc8_dev = best(lambda: enc.encode_utf8_tensors(d_data, d_off, 'ids'), a.reps + 1)
        torch.cuda.synchronize()
        same_enc &= bool(np.array_equal(v[0].cpu().numpy(), ref_vals[0]) and np.array_equal(v[1].cpu().numpy(), ref_vals[1]))
        _, t_enc_today = best(lambda: enc.encode_text(strs, 'ids'), 2)

        # ---- the restore ----
        ref_corpus, t_res16 = ingest_best(lambda e: e.restore_text_flat(enc, units, uoff))
        c, t_res8 = ingest_best(lambda e: e.restore_utf8_batch(enc, data, boff))
        same_res = bool(np.array_equal(c[0], ref_corpus[0]) and np.array_equal(c[1], ref_corpus[1]))
        c, t_res8_dev = ingest_best(lambda e: e.restore_utf8_tensors(enc, d_data, d_off))
        same_res &= bool(np.array_equal(c[0], ref_corpus[0]) and np.array_equal(c[1], ref_corpus[1]))
        _, t_res_today = ingest_best(lambda e: e.restore_text(enc, strs))
        enc.close()

        ms = lambda s: round(s * 1e3, 3)
        res = {
            'what': 'text as UTF-8: bytes transcoded on the device in front of the text pipelines',
            'mix': mix, 'texts': a.texts, 'text_chars': [a.min, a.max], 'bytes': int(data.size),
            'units': int(units.size), 'replaced': int(st['replaced']), 'merges': len(merges),
            'transcode_kernel_ms': ms(k_s), 'transcode_bytes_per_s': data.size / k_s,
            'transcode_hbm_bytes': int(moved), 'transcode_gbs': moved / k_s / 1e9,
            'transcode_frac_hbm_peak': moved / k_s / 1e9 / HBM_PEAK_GBS,
            'd2d_copy_of_read_plus_written_ms': ms(copy_s), 'transcode_over_d2d_copy': k_s / copy_s,
            'transcode_identical_to_python': same_units,
            'add':     {'utf8_host_ms': ms(t_add8), 'utf8_device_ms': ms(t_add8_dev), 'utf16_host_flat_ms': ms(t_add16),
                        'today_decode_ms': ms(t_decode), 'today_add_text_ms': ms(t_add_today),
                        'today_total_ms': ms(t_decode + t_add_today), 'identical': same_add},
            'encode':  {'utf8_host_ms': ms(t_enc8), 'utf8_device_ms': ms(t_enc8_dev), 'utf16_host_flat_ms': ms(t_enc16),
                        'today_decode_ms': ms(t_decode), 'today_encode_text_ms': ms(t_enc_today),
                        'today_total_ms': ms(t_decode + t_enc_today), 'identical': same_enc},
            'restore': {'utf8_host_ms': ms(t_res8), 'utf8_device_ms': ms(t_res8_dev), 'utf16_host_flat_ms': ms(t_res16),
                        'today_decode_ms': ms(t_decode), 'today_restore_text_ms': ms(t_res_today),
                        'today_total_ms': ms(t_decode + t_res_today), 'identical': same_res},
        }
        print(json.dumps(res), flush=True)
        lines.append(json.dumps(res))
        if not (same_units and same_add and same_enc and same_res):
            sys.exit('a UTF-8 route and the UTF-16 form disagree')
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, 'w') as f:
        f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
