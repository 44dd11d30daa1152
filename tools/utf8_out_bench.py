#!/usr/bin/env python3
"""What the UTF-8 back costs (csrc/bpe_utf8_out.hip.h: UTF-16 units -> bytes on the device) and what
the two ways out built on it take, into host and into device buffers.

The batch is tools/utf8_bench.py's: a stretch of the synthetic latin1 stream cut into texts of
[min, max] chars, rendered as UTF-8 in the same four mixes (ascii, cyrillic_cjk, half_supp,
ascii_1pct_bad), ingested from those bytes, trained for --merges merges, and encoded to ids by the
encoder; what is decoded here is that encoder output, and what is exported is that corpus.
One JSON line per mix, printed and written to profiles/utf8_out_bench.jsonl:
  - the transcode's kernel time (HIP events, the decoder's bpe_utf8_stats, device buffers in and out)
    on the decoded units, its ratio to a device-to-device copy of the bytes it writes (torch, CUDA
    events; and of the bytes it reads plus writes, as tools/utf8_bench.py reports it), and its share of
    the 8 TB/s HBM spec peak by its own bytes: 2 reads of each 2-byte unit + the bytes written;
  - beside them the input transcode's figures for the same mix from profiles/utf8_bench.jsonl, when
    that file is there: the yardstick, the same algorithmic shape read the other way;
  - the whole decode_utf8 and export_utf8 calls into host buffers (the flat form) and into device
    buffers (torch tensors), and the decoder's own kernel time inside decode_utf8 (its pipeline runs
    twice per call: the sizing pass, then the units);
  - for comparison, in the same run, what a caller does today: the UTF-16 form (decode, export_text:
    strings) plus str.encode per text on the host; and the UTF-16 flat form alone (units, no strings);
  - whether each route's bytes were identical to that host encode.

Usage: tools/utf8_out_bench.py [--texts 100000] [--min 16] [--max 1024] [--reps 3] [--merges 100]
"""
import argparse
import importlib
import json
import os
import re
import sys
import time

import numpy as np

import torch  # (before libbpe loads: PyTorch's HIP runtime must be the process's first)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))
pkg = importlib.import_module('bpe-tokenizer_amd')
from utf8_bench import HBM_PEAK_GBS, MIXES, best, render  # noqa: E402


LONE = re.compile(rb'\xed[\xa0-\xbf][\x80-\xbf]')   # a lone surrogate as surrogatepass writes it


def host_encode(strs):
    """What Buffer.from(text) writes, per text on the host: lone surrogates become U+FFFD."""
    return [LONE.sub(b'\xef\xbf\xbd', s.encode('utf-8', 'surrogatepass')) for s in strs]


def d2d_copy_s(n_bytes, reps, dev):
    x = torch.empty(max(n_bytes, 1), dtype=torch.uint8, device=dev)
    y = torch.empty_like(x)
    c_ms = []
    for _ in range(reps + 1):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        y.copy_(x)
        e1.record()
        torch.cuda.synchronize()
        c_ms.append(e0.elapsed_time(e1))
    return min(c_ms[1:]) / 1e3


def yardstick(mix):
    """The input transcode's line for the mix (profiles/utf8_bench.jsonl), or None."""
    p = os.path.join(ROOT, 'profiles', 'utf8_bench.jsonl')
    if not os.path.exists(p):
        return None
    for line in open(p):
        r = json.loads(line)
        if r.get('mix') == mix:
            return {'transcode_kernel_ms': r['transcode_kernel_ms'],
                    'transcode_over_d2d_copy': r['transcode_over_d2d_copy'],
                    'transcode_frac_hbm_peak': r['transcode_frac_hbm_peak']}
    return None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--texts', type=int, default=100000)
    ap.add_argument('--min', type=int, default=16)
    ap.add_argument('--max', type=int, default=1024)
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--merges', type=int, default=100)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'utf8_out_bench.jsonl'))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit('utf8_out_bench needs a HIP device')
    dev = torch.device('cuda', 0)
    rng = np.random.default_rng(5)
    text_lens = rng.integers(a.min, a.max + 1, size=a.texts)
    src = pkg.synth_latin1(int(text_lens.sum()), seed=12345, A=256, skip=256 << 20)
    off = np.zeros(a.texts + 1, np.int64)
    np.cumsum(text_lens, out=off[1:])
    lines = []
    for mix in MIXES:
        data, boff = render(mix, src, off, rng)

        # the corpus, the merges, and the encoder's output for the batch
        eng = pkg.Engine(0)
        new_chars, _ = eng.add_utf8_batch(data, boff)
        merges = eng.merge_until(0, 2, a.merges)
        n_chars = len(new_chars)
        abc = [(m[0], m[1], n_chars + i) for i, m in enumerate(merges)]
        enc = pkg.Encoder(0, abc)
        enc.set_chars({int(cp): i for i, cp in enumerate(new_chars)})
        ids, ioff = enc.encode_utf8(data, boff, 'ids')
        enc.close()
        dec = pkg.Decoder(0)
        dec.add_tokens([chr(int(cp)) for cp in new_chars])
        dec.add_merges(abc)
        d_ids, d_ioff = torch.from_numpy(ids.copy()).to(dev), torch.from_numpy(ioff).to(dev)

        # what a caller does today: the UTF-16 form, then an encode per text on the host
        texts_ids = [ids[ioff[k]:ioff[k + 1]] for k in range(a.texts)]
        strs, t_dec16 = best(lambda: dec.decode(texts_ids, 'ids'), 2)
        want, t_encode = best(lambda: host_encode(strs), 1)
        want_flat = np.frombuffer(b''.join(want), np.uint8)
        want_off = np.concatenate([[0], np.cumsum([len(b) for b in want])]).astype(np.int64)
        _, t_dec16_flat = best(lambda: dec.decode_flat(ids, ioff, 'ids'), a.reps + 1)

        # ---- the transcode alone, device buffers in and out ----
        d_units, d_uoff = dec.decode_tensors(d_ids, d_ioff, 'ids')
        n_units = int(d_units.numel())
        out, ooff = dec.utf16_to_utf8_tensors(d_units, d_uoff)   # warm-up
        same_t = bool(np.array_equal(out.cpu().numpy(), want_flat) and np.array_equal(ooff.cpu().numpy(), want_off))
        k_ms = []
        for _ in range(a.reps):
            dec.reset_utf8_stats()
            dec.utf16_to_utf8_tensors(d_units, d_uoff)
            st = dec.utf8_stats()
            k_ms.append(st['kernel_ms'])         # (of the call that wrote its bytes; the wrapper's sizing call is not counted)
        k_s = min(k_ms) / 1e3
        n_bytes = int(want_flat.size)
        moved = 2 * 2 * n_units + n_bytes        # 2 reads of each unit + the bytes written
        copy_out_s = d2d_copy_s(n_bytes, a.reps, dev)
        copy_rw_s = d2d_copy_s(2 * n_units + n_bytes, a.reps, dev)

        # ---- decode_utf8 ----
        dec.reset_stats()
        v, t_dec8 = best(lambda: dec.decode_utf8_flat(ids, ioff, 'ids'), a.reps + 1)
        dec_kernel_ms = dec.stats()['kernel_ms'] / (a.reps + 1)
        same_dec = bool(np.array_equal(v[0], want_flat) and np.array_equal(v[1], want_off))
        v, t_dec8_dev = best(lambda: dec.decode_utf8_tensors(d_ids, d_ioff, 'ids'), a.reps + 1)
        torch.cuda.synchronize()
        same_dec &= bool(np.array_equal(v[0].cpu().numpy(), want_flat) and np.array_equal(v[1].cpu().numpy(), want_off))

        # ---- export_utf8: the trained corpus (the batch's texts, merged) ----
        xstrs, t_exp16 = best(lambda: eng.export_text(dec), 2)
        xwant, t_xencode = best(lambda: host_encode(xstrs), 1)
        xflat = np.frombuffer(b''.join(xwant), np.uint8)
        _, t_exp16_flat = best(lambda: eng.export_text_flat(dec), a.reps + 1)
        v, t_exp8 = best(lambda: eng.export_utf8_flat(dec), a.reps + 1)
        same_exp = bool(np.array_equal(v[0], xflat))
        v, t_exp8_dev = best(lambda: eng.export_utf8_tensors(dec), a.reps + 1)
        torch.cuda.synchronize()
        same_exp &= bool(np.array_equal(v[0].cpu().numpy(), xflat))
        same_exp &= bool(np.array_equal(xflat, want_flat))   # (the corpus holds the batch's texts)
        eng.close()
        dec.close()

        ms = lambda s: round(s * 1e3, 3)
        res = {
            'what': 'text out as UTF-8: units transcoded on the device behind the decode and the export',
            'mix': mix, 'texts': a.texts, 'text_chars': [a.min, a.max], 'ids': int(ids.size), 'units': n_units,
            'bytes': n_bytes, 'replaced': int(st['replaced']), 'merges': len(merges),
            'transcode_kernel_ms': ms(k_s), 'transcode_bytes_out_per_s': n_bytes / k_s,
            'transcode_hbm_bytes': int(moved), 'transcode_gbs': moved / k_s / 1e9,
            'transcode_frac_hbm_peak': moved / k_s / 1e9 / HBM_PEAK_GBS,
            'd2d_copy_of_written_ms': ms(copy_out_s), 'transcode_over_d2d_copy_of_written': k_s / copy_out_s,
            'd2d_copy_of_read_plus_written_ms': ms(copy_rw_s), 'transcode_over_d2d_copy': k_s / copy_rw_s,
            'utf8_in_yardstick': yardstick(mix),
            'transcode_identical_to_host_encode': same_t,
            'decode': {'utf8_host_ms': ms(t_dec8), 'utf8_device_ms': ms(t_dec8_dev),
                       'decoder_kernel_ms_per_utf8_call': round(dec_kernel_ms, 3),
                       'utf16_host_flat_ms': ms(t_dec16_flat), 'today_decode_ms': ms(t_dec16),
                       'today_encode_per_text_ms': ms(t_encode), 'today_total_ms': ms(t_dec16 + t_encode),
                       'identical': same_dec},
            'export': {'utf8_host_ms': ms(t_exp8), 'utf8_device_ms': ms(t_exp8_dev),
                       'utf16_host_flat_ms': ms(t_exp16_flat), 'today_export_text_ms': ms(t_exp16),
                       'today_encode_per_text_ms': ms(t_xencode), 'today_total_ms': ms(t_exp16 + t_xencode),
                       'identical': same_exp},
        }
        print(json.dumps(res), flush=True)
        lines.append(json.dumps(res))
        if not (same_t and same_dec and same_exp):
            sys.exit('a UTF-8 route and the host encode disagree')
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, 'w') as f:
        f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
