#!/usr/bin/env python3
"""Writes tests/golden/utf8_cases.json: UTF-8 inputs and the UTF-16 units Node's own decoder
(Buffer.prototype.toString(), the WHATWG UTF-8 decode with U+FFFD replacement) gives for each.

Inputs
  exhaustive  every string of length 0..3 over the 27 range-edge bytes (EDGE), in
              itertools.product order, shortest first; not stored, rebuilt from the rule
              (cases() below, which tests/test_utf8.py imports);
  random      2 000 strings of length 4..12 over the same bytes, as byte lists;
  wellformed  500 well-formed strings mixing ASCII, Cyrillic, CJK, emoji, a BOM and U+FFFD itself,
              as byte lists.
Expected output, for the cases in that order: `lens` (units per case) and `units` (all units back to
back), each a little-endian uint16 array, zlib-compressed and base64-encoded so that the file stays
well under 300 KB.

Usage: python tools/gen_utf8_golden.py   (needs `node` on the PATH)
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
OUT = os.path.join(ROOT, 'tests', 'golden', 'utf8_cases.json')
EDGE = bytes.fromhex('00417f808f909fa0bfc0c1c2dfe0e1ecedeeeff0f1f3f4f5f7f8ff')
MAX_LEN = 3
SEED = 20240607

NODE = r"""
const fs = require('fs');
const inputs = JSON.parse(fs.readFileSync(process.argv[2], 'utf8'));
const out = inputs.map(h => Buffer.from(Buffer.from(h, 'hex').toString(), 'utf16le').toString('hex'));
fs.writeFileSync(process.argv[3], JSON.stringify(out));
"""


def exhaustive(alphabet=EDGE, max_len=MAX_LEN):
    return [bytes(t) for n in range(max_len + 1) for t in itertools.product(alphabet, repeat=n)]


def make_random(rng):
    return [bytes(rng.choice(EDGE) for _ in range(rng.randint(4, 12))) for _ in range(2000)]


def make_wellformed(rng):
    pools = ['abcXYZ 019.,\n', '\u041f\u0440\u0438\u0432\u0435\u0442\u043c\u0438\u0440\u0451\u0436', '\u6f22\u5b57\u4eee\u540d\u4ea4\u3058\u308a\u6587',
             '\U0001f600\U0001f389\U0001f680\U00010348', '\ufeff', '\ufffd', '\u00e9\u07ff\u0800\uffff\U00010000\U0010ffff']
    out = []
    for _ in range(500):
        s = ''.join(rng.choice(rng.choice(pools)) for _ in range(rng.randint(1, 12)))
        out.append(s.encode('utf-8'))
    return out


def cases(fixture):
    """Every input of a loaded fixture, in the order of its expected output."""
    return (exhaustive(bytes(fixture['alphabet']), fixture['exhaustive_max_len']) +
            [bytes(x) for x in fixture['random']] + [bytes(x) for x in fixture['wellformed']])


def expected(fixture):
    """Per case, the uint16 array of units Node decoded it to."""
    def arr(key):
        return np.frombuffer(zlib.decompress(base64.b64decode(fixture[key])), dtype='<u2')
    lens, units = arr('lens'), arr('units')
    ends = np.cumsum(lens.astype(np.int64))
    return [units[e - n:e] for e, n in zip(ends, lens)]


def main():
    rng = random.Random(SEED)
    fixture = {
        'decoder': 'node %s Buffer.prototype.toString()' % subprocess.check_output(['node', '--version']).decode().strip(),
        'alphabet': list(EDGE), 'exhaustive_max_len': MAX_LEN,
        'random': [list(b) for b in make_random(rng)],
        'wellformed': [list(b) for b in make_wellformed(rng)],
    }
    inputs = cases(fixture)
    with tempfile.TemporaryDirectory() as tmp:
        src, dst, js = (os.path.join(tmp, n) for n in ('in.json', 'out.json', 'decode.js'))
        json.dump([b.hex() for b in inputs], open(src, 'w'))
        open(js, 'w').write(NODE)
        subprocess.check_call(['node', js, src, dst])
        decoded = [np.frombuffer(bytes.fromhex(h), dtype='<u2') for h in json.load(open(dst))]
    assert len(decoded) == len(inputs)

    def pack(a):
        return base64.b64encode(zlib.compress(np.asarray(a, dtype='<u2').tobytes(), 9)).decode()
    fixture['lens'] = pack([len(d) for d in decoded])
    fixture['units'] = pack(np.concatenate(decoded))
    fixture['n_cases'] = len(inputs)
    with open(OUT, 'w') as f:
        json.dump(fixture, f, separators=(',', ':'))
    size = os.path.getsize(OUT)
    print('%s: %d cases, %d bytes' % (OUT, len(inputs), size))
    assert size < 300 * 1000, 'the fixture must stay under 300 KB'


if __name__ == '__main__':
    sys.exit(main())
