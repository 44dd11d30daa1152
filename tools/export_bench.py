#!/usr/bin/env python3
"""Throughput of the corpus export (bpe_export_samples, bpe_export_text_batch, csrc/bpe_export.hip.h)
against what reads a corpus back today (read_corpus, read_samples).

The corpus is synth_latin1 at --mib MiB in 1 MiB samples.  It is timed twice in one run: after
--merges merges (dead slots present) and again right after a compaction (an empty sample is appended:
the append packs the corpus first).  Per state one JSON line, printed and written to
profiles/export_bench.jsonl (one warm-up call, then --reps calls; min, median and max):
  (a) read_corpus as it stands;
  (b) the host form of the export, ids;
  (c) the host form, codes;
  (d) the device forms: ids, vectors and codes, into tensors made before the clock starts;
  (e) export_text_tensors through a decoder of the corpus's tokens;
  (f) a device-to-device copy of the bytes (d) writes (4 B, and 2 B for codes, per token);
  (g) read_samples against the selected form (host) on a random 1 % of the samples;
with the kernels' time (export_stats) against (f), their bytes by their shape (the region census and
the walk read every slot once each, 4 B; the walk writes one value per token and 8 B per sample) as a
share of the 8 TB/s spec peak, and whether every route gave the same output.
A last line times the 100 000-text batch of tools/restore_text_bench.py: restored into a fresh
context, then exported as ids, as text on the device, and read back by read_corpus.

Usage: tools/export_bench.py [--mib 256] [--merges 500] [--reps 3] [--texts 100000]
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
CHUNK = pkg.EXPORT_TILE


def spread(xs):
    xs = sorted(xs)
    return {'min': xs[0] * 1e3, 'median': xs[len(xs) // 2] * 1e3, 'max': xs[-1] * 1e3, 'reps': len(xs)}


def timed(fn, reps, e=None):
    """(the last result, wall times, the export kernels' times) of reps calls after one warm-up."""
    out = fn()
    ts, ks = [], []
    for _ in range(reps):
        if e is not None:
            e.reset_export_stats()
        t0 = time.perf_counter()
        out = fn()
        ts.append(time.perf_counter() - t0)
        if e is not None:
            ks.append(e.export_stats()['kernel_ms'] / 1e3)
    return out, ts, ks


def vector_index(e):
    """to_vector_index of compactVectorIndex from the engine's own counts: -1 for an absent token."""
    counts = e.token_counts()
    return np.where(counts > 0, np.cumsum(counts > 0) - 1, -1).astype(np.int32)


def decoder_of(cmap, n_tok, abc):
    chars = [''] * n_tok
    for b in range(256):
        if cmap[b] >= 0:
            chars[int(cmap[b])] = chr(b)
    dec = pkg.Decoder(0)
    dec.add_tokens(chars)
    if len(abc):
        dec.add_merges(abc)
    return dec


def measure(e, dec, state, slots, reps, dev, rng):
    ns, n_live = e.corpus_size()
    index = vector_index(e)
    res = {'state': state, 'samples': ns, 'tokens': n_live, 'slots_streamed': slots}
    # (a) read_corpus as it stands
    (ids_a, off_a), t_a, _ = timed(e.read_corpus, max(1, reps - 1))
    # (b), (c) the host forms
    (ids_b, off_b), t_b, k_b = timed(lambda: e.export_samples(None, 'ids'), reps, e)
    (code_c, off_c), t_c, _ = timed(lambda: e.export_samples(None, 'code'), reps, e)
    same = bool(np.array_equal(ids_a, ids_b) and np.array_equal(off_a, off_b) and np.array_equal(off_a, off_c)
                and np.array_equal(code_c, (ids_a + 1).astype(np.uint16)))
    want_vec = index[ids_a]
    del ids_b, code_c
    # (d) the device forms
    dev_ms, ker_ms = {}, {}
    for kind in ('ids', 'vectors', 'code'):
        out = torch.empty(n_live, dtype=torch.int16 if kind == 'code' else torch.int32, device=dev)
        tvi = index if kind == 'vectors' else None
        (vals, off), ts, ks = timed(lambda: e.export_samples_tensors(None, kind, tvi, out=out), reps, e)
        dev_ms[kind], ker_ms[kind] = ts, ks
        host = vals.cpu().numpy()
        want = {'ids': ids_a, 'vectors': want_vec, 'code': (ids_a + 1).astype(np.uint16).view(np.int16)}[kind]
        same = same and bool(np.array_equal(host, want) and np.array_equal(off.cpu().numpy(), off_a))
        del out, vals, host
    # (e) text on the device; checked against the decoder's own host form on the first 4 samples
    (units, uoff), t_e, k_e = timed(lambda: e.export_text_tensors(dec), reps, e)
    few = min(ns, 4)
    want_u, want_o = dec.decode_flat(ids_a[:off_a[few]], off_a[:few + 1], 'ids')
    o = uoff.cpu().numpy()
    same = same and bool(np.array_equal(o[:few + 1], want_o) and
                         np.array_equal(units[:o[few]].cpu().numpy().view(np.uint16), want_u))
    n_units = int(o[-1])
    del units, uoff
    # (f) device-to-device copies of the bytes (d) writes
    t_f = {}
    for kind, dt in (('ids', torch.int32), ('code', torch.int16)):
        src = torch.zeros(n_live, dtype=dt, device=dev)
        dst = torch.empty_like(src)
        ts = []
        for _ in range(reps + 1):
            ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            ev0.record()
            dst.copy_(src)
            ev1.record()
            torch.cuda.synchronize(dev)
            ts.append(ev0.elapsed_time(ev1) / 1e3)
        t_f[kind] = ts[1:]
        del src, dst
    # (g) a random 1 % of the samples: read_samples against the selected form
    pick = rng.choice(ns, size=max(1, ns // 100), replace=False)
    (ids_g, off_g), t_g0, _ = timed(lambda: e.read_samples(pick), reps)
    (ids_s, off_s), t_g1, k_g = timed(lambda: e.export_samples(pick, 'ids'), reps, e)
    same = same and bool(np.array_equal(ids_g, ids_s) and np.array_equal(off_g, off_s))
    want_g = np.concatenate([ids_a[off_a[i]:off_a[i + 1]] for i in pick])
    same = same and bool(np.array_equal(ids_s, want_g))

    def kernel(kind, esize):
        k = min(ker_ms[kind])
        hbm = 8 * slots + esize * n_live + 8 * ns     # census + walk reads, the values and offsets written
        return {'ms': spread(ker_ms[kind]), 'hbm_bytes': int(hbm), 'gbs': hbm / k / 1e9,
                'frac_hbm_peak': hbm / k / 1e9 / HBM_PEAK_GBS,
                'over_d2d_copy': k / min(t_f['code' if esize == 2 else 'ids'])}
    res.update({
        'read_corpus_ms': spread(t_a),
        'host_ids_ms': spread(t_b), 'host_ids_kernel_ms': spread(k_b), 'host_code_ms': spread(t_c),
        'host_ids_over_read_corpus': min(t_b) / min(t_a),
        'device_ids_ms': spread(dev_ms['ids']), 'device_vectors_ms': spread(dev_ms['vectors']),
        'device_code_ms': spread(dev_ms['code']),
        'kernels_ids': kernel('ids', 4), 'kernels_vectors': kernel('vectors', 4), 'kernels_code': kernel('code', 2),
        'text_tensors_ms': spread(t_e), 'text_units': n_units, 'text_export_kernel_ms': spread(k_e),
        'd2d_copy_ids_ms': spread(t_f['ids']), 'd2d_copy_ids_bytes': 4 * n_live,
        'd2d_copy_code_ms': spread(t_f['code']), 'd2d_copy_code_bytes': 2 * n_live,
        'selected': {'samples': int(pick.size), 'tokens': int(ids_s.size), 'read_samples_ms': spread(t_g0),
                     'export_samples_ms': spread(t_g1), 'export_kernel_ms': spread(k_g),
                     'export_over_read_samples': min(t_g1) / min(t_g0)},
        'identical_outputs': same,
    })
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--mib', type=int, default=256)
    ap.add_argument('--merges', type=int, default=500)
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--texts', type=int, default=100000)
    ap.add_argument('--text-merges', type=int, default=8000)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'export_bench.jsonl'))
    a = ap.parse_args()
    if torch is None or not torch.cuda.is_available():
        sys.exit('the device forms and (f) need torch with a HIP device')
    dev = torch.device('cuda', 0)
    rng = np.random.default_rng(7)
    lines = []

    n = a.mib << 20
    data = pkg.synth_latin1(n, seed=12345, A=256)
    e = pkg.Engine(0)
    e.stats_enable(True)
    cmap, n_tok, _ = e.add_latin1(data, sample_bytes=1 << 20)
    got = e.merge_until(0, 2, a.merges)
    abc = np.asarray([(x, y, n_tok + k) for k, (x, y, _w) in enumerate(got)], np.int32)
    dec = decoder_of(cmap, n_tok, abc)
    st = e.stats()
    # slots a pass streams now: those of the last compaction less nothing (merges only kill slots in
    # place), i.e. the live slots then; without one, the ingest's
    ns, n_live = e.corpus_size()
    slots_dead = n + ns if st['compactions'] == 0 else None
    for state in ('dead', 'packed'):
        if state == 'packed':
            e.add_sample([])                 # (the append packs the corpus first)
        ns, n_live = e.corpus_size()
        chunks = -(-(n_live + ns) // CHUNK)
        slots = chunks * CHUNK if state == 'packed' or slots_dead is None else -(-slots_dead // CHUNK) * CHUNK
        res = {'what': 'corpus out on the device (bpe_export_samples, bpe_export_text_batch)', 'mib': a.mib,
               'merges': len(got), 'compactions_while_merging': st['compactions'],
               'slots_streamed_is_lower_bound': state == 'dead' and slots_dead is None}
        res.update(measure(e, dec, state, slots, a.reps, dev, rng))
        print(json.dumps(res), flush=True)
        lines.append(json.dumps(res))
        if not res['identical_outputs']:
            sys.exit('the routes disagree')
    e.close()
    dec.close()

    # the 100 000-text batch of tools/restore_text_bench.py, restored and exported
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    from restore_text_bench import train
    text_lens = np.random.default_rng(5).integers(16, 1025, size=a.texts)
    cmap, n_tok, abc, rest = train('uniform', n, int(text_lens.sum()), a.text_merges)
    off = np.zeros(a.texts + 1, np.int64)
    np.cumsum(text_lens, out=off[1:])
    off = np.minimum(off, rest.size)
    units = rest[:off[-1]].astype(np.uint16)
    enc = pkg.Encoder(0, abc)
    enc.set_chars({int(ch): int(cmap[ch]) for ch in range(256) if cmap[ch] >= 0})
    dec = decoder_of(cmap, n_tok, abc)
    e = pkg.Engine(0)
    e.restore_text_flat(enc, units, off)
    ns, n_live = e.corpus_size()
    (ids_a, off_a), t_a, _ = timed(e.read_corpus, a.reps)
    (ids_b, off_b), t_b, _ = timed(lambda: e.export_samples(None, 'ids'), a.reps, e)
    out = torch.empty(n_live, dtype=torch.int32, device=dev)
    (vals, doff), t_d, k_d = timed(lambda: e.export_samples_tensors(None, 'ids', out=out), a.reps, e)
    (tu, to), t_e, _ = timed(lambda: e.export_text_tensors(dec), a.reps, e)
    texts_back = tu.cpu().numpy().view(np.uint16)
    same = bool(np.array_equal(ids_a, ids_b) and np.array_equal(off_a, off_b) and
                np.array_equal(vals.cpu().numpy(), ids_a) and np.array_equal(texts_back, units) and
                np.array_equal(to.cpu().numpy(), off - off[0]))
    res = {'what': 'the 100 000-text batch of tools/restore_text_bench.py, restored, then exported',
           'texts': ns, 'units': int(units.size), 'tokens': n_live, 'merges': int(len(abc)),
           'read_corpus_ms': spread(t_a), 'host_ids_ms': spread(t_b), 'device_ids_ms': spread(t_d),
           'device_ids_kernel_ms': spread(k_d), 'text_tensors_ms': spread(t_e),
           'host_ids_over_read_corpus': min(t_b) / min(t_a), 'identical_outputs': same,
           'text_equals_the_restored_texts': bool(np.array_equal(texts_back, units))}
    print(json.dumps(res), flush=True)
    lines.append(json.dumps(res))
    with open(a.out, 'w') as f:
        f.write('\n'.join(lines) + '\n')
    if not same:
        sys.exit('the routes disagree')


if __name__ == '__main__':
    main()
