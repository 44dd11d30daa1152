#!/usr/bin/env python3
"""Writes tests/golden/utf8_out_cases.json: JS strings (as UTF-16 code units) and the bytes Node's
own encoder (Buffer.from(str, 'utf8'): the WHATWG conversion to a USVString, then UTF-8) gives for
each.

Inputs
  exhaustive  every string of length 0..3 over the 14 edge units (EDGE), in itertools.product
              order, shortest first; not stored, rebuilt from the rule (cases() below, which
              tests/test_utf8_out.py imports);
  random      400 strings of length 4..16, two thirds of their units surrogates, as unit lists.
Expected output, for the cases in that order: `lens` (bytes per case, little-endian uint16) and
`bytes` (all bytes back to back), zlib-compressed and base64-encoded so that the file stays well
under 300 KB.

Usage: python tools/gen_utf8_out_golden.py   (needs `node` on the PATH)
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
OUT = os.path.join(ROOT, 'tests', 'golden', 'utf8_out_cases.json')
EDGE = [0x00, 0x7F, 0x80, 0x7FF, 0x800, 0xD7FF, 0xD800, 0xDBFF, 0xDC00, 0xDFFF, 0xE000, 0xFEFF, 0xFFFD, 0xFFFF]
MAX_LEN = 3
SEED = 20240611

NODE = r"""
const fs = require('fs');
const inputs = JSON.parse(fs.readFileSync(process.argv[2], 'utf8'));
const out = inputs.map(units => Buffer.from(String.fromCharCode(...units), 'utf8').toString('hex'));
fs.writeFileSync(process.argv[3], JSON.stringify(out));
"""


def exhaustive(alphabet=EDGE, max_len=MAX_LEN):
    return [list(t) for n in range(max_len + 1) for t in itertools.product(alphabet, repeat=n)]


def make_random(rng):
    def unit():
        r = rng.random()
        if r < 0.33:
            return rng.randrange(0xD800, 0xDC00)
        if r < 0.66:
            return rng.randrange(0xDC00, 0xE000)
        return rng.choice([rng.randrange(0x80), rng.randrange(0x80, 0x800), rng.randrange(0x800, 0xD800),
                           rng.randrange(0xE000, 0x10000)])
    return [[unit() for _ in range(rng.randint(4, 16))] for _ in range(400)]


def cases(fixture):
    """Every input of a loaded fixture (a list of unit lists), in the order of its expected output."""
    return exhaustive(fixture['alphabet'], fixture['exhaustive_max_len']) + [list(x) for x in fixture['random']]


def expected(fixture):
    """Per case, the bytes Node encoded it to."""
    lens = np.frombuffer(zlib.decompress(base64.b64decode(fixture['lens'])), dtype='<u2')
    data = zlib.decompress(base64.b64decode(fixture['bytes']))
    ends = np.cumsum(lens.astype(np.int64))
    return [data[e - n:e] for e, n in zip(ends, lens)]


def main():
    rng = random.Random(SEED)
    fixture = {
        'encoder': 'node %s Buffer.from(str, "utf8")' % subprocess.check_output(['node', '--version']).decode().strip(),
        'alphabet': EDGE, 'exhaustive_max_len': MAX_LEN,
        'random': make_random(rng),
    }
    inputs = cases(fixture)
    with tempfile.TemporaryDirectory() as tmp:
        src, dst, js = (os.path.join(tmp, n) for n in ('in.json', 'out.json', 'encode.js'))
        json.dump(inputs, open(src, 'w'))
        open(js, 'w').write(NODE)
        subprocess.check_call(['node', js, src, dst])
        encoded = [bytes.fromhex(h) for h in json.load(open(dst))]
    assert len(encoded) == len(inputs)
    fixture['lens'] = base64.b64encode(zlib.compress(np.asarray([len(b) for b in encoded], '<u2').tobytes(), 9)).decode()
    fixture['bytes'] = base64.b64encode(zlib.compress(b''.join(encoded), 9)).decode()
    fixture['n_cases'] = len(inputs)
    with open(OUT, 'w') as f:
        json.dump(fixture, f, separators=(',', ':'))
    size = os.path.getsize(OUT)
    print('%s: %d cases, %d bytes' % (OUT, len(inputs), size))
    assert size < 300 * 1000, 'the fixture must stay under 300 KB'


if __name__ == '__main__':
    sys.exit(main())
