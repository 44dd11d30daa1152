#!/usr/bin/env python3
"""Writes tests/golden/lines_cases.json: JS strings (as UTF-16 code units) and the samples the
drop-in's host-only corpus helpers (js/core.js: linesToCorpus, linesTrimmedToCorpus,
fileContentToCorpus, pinned by tests/js/host_only.js) make of each, run by Node.

Inputs
  exhaustive  every string of length 0..4 over the 15 units of ALPHABET, in itertools.product
              order, shortest first; not stored, rebuilt from the rule (cases() below, which
              tests/test_lines.py imports);
  random      1 000 seeded strings of length 5..40 over the same alphabet;
  long        200 longer mixed-script texts (Latin, Cyrillic, CJK, pairs; LF and CR LF line ends,
              runs of the whitespace units).
Expected output per mode ('trim', 'keep', 'file'), for the cases in that order.  Every sample Node
made is a marker, a substring of its input and a marker, so it is stored as where that substring
lies: `first` and `last` (the mode's two markers), `counts` (samples per case), and per sample `gaps`
(input units between the end of the sample before it and its start) and `lens` (its units without the
markers).  main() checks that expected() rebuilds Node's samples unit for unit before it writes the
file, which is what keeps every case of the exhaustive part within a few KB.  Arrays are uint16,
little-endian, zlib-compressed and base64-encoded like tests/golden/utf8_cases.json; the stored inputs
likewise (`lens` uint32).

Usage: python tools/gen_lines_golden.py   (needs `node` on the PATH)
"""
import base64
import itertools
import json
import os
import random
import subprocess
import sys
import tempfile
import zlib

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, 'tests', 'golden', 'lines_cases.json')
# a, space, \t, \r, \n, NBSP, NEL, U+180E, U+200B, LS, ideographic space, BOM, FS, a high and a low surrogate
ALPHABET = [0x61, 0x20, 0x09, 0x0D, 0x0A, 0xA0, 0x85, 0x180E, 0x200B, 0x2028, 0x3000, 0xFEFF, 0x1C, 0xD83D, 0xDE00]
MAX_LEN = 4
SEED = 20240918
MODES = ('trim', 'keep', 'file')
HELPERS = {'trim': 'linesToCorpus', 'keep': 'linesTrimmedToCorpus', 'file': 'fileContentToCorpus'}

NODE = r"""
const fs = require('fs');
const core = require(process.argv[2]);
const dir = process.argv[3];
const lens = new Uint32Array(fs.readFileSync(dir + '/in_lens.bin').buffer.slice(0));
const raw = fs.readFileSync(dir + '/in_units.bin');
const units = new Uint16Array(raw.buffer.slice(raw.byteOffset, raw.byteOffset + raw.length));
const texts = [];
let at = 0;
for (const n of lens) {
  let s = '';
  for (let i = at; i < at + n; i += 4096) s += String.fromCharCode.apply(null, units.subarray(i, Math.min(i + 4096, at + n)));
  texts.push(s);
  at += n;
}
const helpers = {trim: core.linesToCorpus, keep: core.linesTrimmedToCorpus, file: t => [core.fileContentToCorpus(t)]};
for (const mode of Object.keys(helpers)) {
  const counts = [], slens = [], parts = [];
  for (const t of texts) {
    const samples = helpers[mode](t);
    counts.push(samples.length);
    for (const s of samples) {
      slens.push(s.length);
      const u = new Uint16Array(s.length);
      for (let i = 0; i < s.length; i++) u[i] = s.charCodeAt(i);
      parts.push(Buffer.from(u.buffer));
    }
  }
  fs.writeFileSync(dir + '/' + mode + '_counts.bin', Buffer.from(new Uint32Array(counts).buffer));
  fs.writeFileSync(dir + '/' + mode + '_lens.bin', Buffer.from(new Uint32Array(slens).buffer));
  fs.writeFileSync(dir + '/' + mode + '_units.bin', Buffer.concat(parts));
}
"""


def exhaustive(alphabet=ALPHABET, max_len=MAX_LEN):
    return [list(t) for n in range(max_len + 1) for t in itertools.product(alphabet, repeat=n)]


def make_random(rng):
    return [[rng.choice(ALPHABET) for _ in range(rng.randint(5, 40))] for _ in range(1000)]


WORDS = ['the', 'quick', 'brown', 'fox', 'jumps', 'over', 'lazy', 'dog', 'съешь', 'ещё', 'этих', 'мягких',
         'французских', 'булок', 'да', 'выпей', 'чаю', '我能吞下', '玻璃', '而不伤', '身体', '\U0001F600', '\U0001F680x',
         'naïve', 'café', '0123', '.', ',', '—']
SPACES = [0x20, 0x20, 0x20, 0x09, 0xA0, 0x3000, 0x2003, 0x2028, 0xFEFF, 0x0B, 0x0C, 0x1680, 0x202F, 0x205F, 0x2029]
NOT_SPACES = [0x85, 0x180E, 0x200B, 0x1C, 0x1F, 0xD83D, 0xDE00]


def make_long(rng):
    texts = []
    for _ in range(200):
        out = []
        for _ in range(rng.randint(2, 8)):                      # lines
            if rng.random() < 0.15:
                out += [rng.choice(SPACES) for _ in range(rng.randint(0, 12))]   # a blank line
            else:
                out += [rng.choice(SPACES) for _ in range(rng.choice([0, 0, 1, 2, 4, 9]))]
                for _ in range(rng.randint(1, 8)):
                    w = rng.choice(WORDS)
                    out += list(np.frombuffer(w.encode('utf-16-le'), '<u2'))
                    out += [rng.choice(SPACES) if rng.random() < 0.9 else rng.choice(NOT_SPACES)]
                out += [rng.choice(SPACES) for _ in range(rng.choice([0, 0, 1, 3, 7]))]
            r = rng.random()
            out += [0x0A] if r < 0.55 else [0x0D, 0x0A] if r < 0.9 else [0x0D] if r < 0.95 else [0x0D, 0x0D, 0x0A]
        if rng.random() < 0.5:
            out.pop()                                            # (no final line end)
        texts.append([int(x) for x in out])
    return texts


def pack(arr, dtype):
    return base64.b64encode(zlib.compress(np.asarray(arr, dtype).tobytes(), 9)).decode()


def unpack(s, dtype):
    return np.frombuffer(zlib.decompress(base64.b64decode(s)), dtype)


def stored(fixture, key):
    lens = unpack(fixture[key + '_lens'], '<u4').astype(np.int64)
    units = unpack(fixture[key + '_units'], '<u2')
    ends = np.cumsum(lens)
    return [units[e - n:e].tolist() for e, n in zip(ends, lens)]


def cases(fixture):
    """Every input of a loaded fixture (a list of unit lists), in the order of its expected output."""
    return exhaustive(fixture['alphabet'], fixture['exhaustive_max_len']) + stored(fixture, 'random') + \
        stored(fixture, 'long')


def expected(fixture, mode, inputs=None):
    """Per case, the list of samples (uint16 arrays) Node's helper made of it."""
    inputs = cases(fixture) if inputs is None else inputs
    counts, gaps, lens = (unpack(fixture['%s_%s' % (mode, k)], '<u2').astype(np.int64) for k in ('counts', 'gaps', 'lens'))
    first, last = fixture[mode + '_first'], fixture[mode + '_last']
    out, j = [], 0
    for t, n in zip(inputs, counts):
        at, samples = 0, []
        for gap, length in zip(gaps[j:j + n], lens[j:j + n]):
            at += gap
            samples.append(np.asarray([first] + list(t[at:at + length]) + [last], np.uint16))
            at += length
        out.append(samples)
        j += n
    return out


def describe(inputs, node):
    """Node's samples of one mode -> (first, last, counts, gaps, lens)."""
    first, last = int(node[0][0][0]), int(node[0][0][-1])
    counts, gaps, lens = [], [], []
    for t, samples in zip(inputs, node):
        counts.append(len(samples))
        at, line = 0, 0                       # the end of the sample before, the start of this line
        for s in samples:
            body = [int(u) for u in s[1:-1]]
            assert s[0] == first and s[-1] == last
            start = line
            while body and t[start:start + len(body)] != body:
                start += 1
                assert start + len(body) <= len(t)
            gaps.append(start - at)
            lens.append(len(body))
            at = start + len(body)
            line = t.index(0x0A, line) + 1 if 0x0A in t[line:] and first != 0x1C else len(t)
    return first, last, counts, gaps, lens


def main():
    rng = random.Random(SEED)
    rnd, lng = make_random(rng), make_long(rng)
    fixture = {
        'helpers': 'node %s, js/core.js %s' % (subprocess.check_output(['node', '--version']).decode().strip(),
                                               ', '.join(HELPERS[m] for m in MODES)),
        'alphabet': ALPHABET, 'exhaustive_max_len': MAX_LEN,
    }
    for key, texts in (('random', rnd), ('long', lng)):
        fixture[key + '_lens'] = pack([len(t) for t in texts], '<u4')
        fixture[key + '_units'] = pack([u for t in texts for u in t], '<u2')
    inputs = cases(fixture)
    with tempfile.TemporaryDirectory() as tmp:
        np.asarray([len(t) for t in inputs], '<u4').tofile(os.path.join(tmp, 'in_lens.bin'))
        np.asarray([u for t in inputs for u in t], '<u2').tofile(os.path.join(tmp, 'in_units.bin'))
        js = os.path.join(tmp, 'run.js')
        open(js, 'w').write(NODE)
        subprocess.check_call(['node', js, os.path.join(ROOT, 'bpe-tokenizer_amd', 'js', 'core.js'), tmp])
        for mode in MODES:
            counts, lens, units = (np.fromfile(os.path.join(tmp, '%s_%s.bin' % (mode, part)), dtype)
                                   for part, dtype in (('counts', '<u4'), ('lens', '<u4'), ('units', '<u2')))
            ends = np.cumsum(lens.astype(np.int64))
            samples = [units[e - n:e] for e, n in zip(ends, lens)]
            cends = np.cumsum(counts.astype(np.int64))
            node = [samples[e - n:e] for e, n in zip(cends, counts)]
            first, last, c, g, ln = describe(inputs, node)
            fixture[mode + '_first'], fixture[mode + '_last'] = first, last
            for key, arr in (('counts', c), ('gaps', g), ('lens', ln)):
                assert max(arr) < 65536
                fixture['%s_%s' % (mode, key)] = pack(arr, '<u2')
            back = expected(fixture, mode, inputs)
            assert all(len(x) == len(y) and all(np.array_equal(p, q) for p, q in zip(x, y))
                       for x, y in zip(back, node)), mode
    fixture['n_cases'] = len(inputs)
    with open(OUT, 'w') as f:
        json.dump(fixture, f, separators=(',', ':'))
    size = os.path.getsize(OUT)
    print('%s: %d cases, %d bytes' % (OUT, len(inputs), size))
    assert size < 100 * 1000, 'the fixture must stay well under the size limit'


if __name__ == '__main__':
    sys.exit(main())
