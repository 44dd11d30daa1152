#!/usr/bin/env python3
"""Writes tests/golden/skipgram_cases.json: small integer arrays and the (target, context) pairs the
reference's own loop makes of them.

The loop is cut out of the reference's example/skip-gram.ts (lines 30-47: `for (let i = 0; ...`
over `tokens` with `window_size`) when this script runs; nothing of it is kept here.  Its one
statement with an effect builds a training record for a network library; the line above it, which
the reference left as a comment, pushes the bare pair onto `dataset`.  The cut keeps that line,
uncommented, in place of the statement, and Node runs the result as it stands.

Cases: for window_size 1, 2, 3 and 5, every length 0..12 and the lengths 2w - 1 .. 2w + 3 (where the
head and the tail of a text stop overlapping), with distinct values so that an error of order shows.

Usage: python tools/gen_skipgram_golden.py PATH/TO/reference   (needs `node` on the PATH)
"""
import json
import os
import random
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, 'tests', 'golden', 'skipgram_cases.json')
SOURCE = ('example', 'skip-gram.ts')
FIRST, LAST = 30, 47          # the loop's lines, 1-based, inclusive
WINDOWS = (1, 2, 3, 5)
SEED = 20240930

HARNESS = r"""
const fs = require('fs');
function run(tokens, window_size) {
  let dataset = [];
  %s
  return dataset;
}
const cases = JSON.parse(fs.readFileSync(process.argv[2], 'utf8'));
fs.writeFileSync(process.argv[3], JSON.stringify(cases.map(c => run(c.values, c.window))));
"""


def cut_loop(path):
    """Lines FIRST..LAST of the file, the commented `dataset.push` line live and the statement after
    it (up to the line that closes its brackets) gone."""
    lines = open(path).read().split('\n')[FIRST - 1:LAST]
    at = [k for k, ln in enumerate(lines) if re.match(r'\s*//\s*dataset\.push\(', ln)]
    assert len(at) == 1 and lines[0].lstrip().startswith('for (') and 'tokens.length' in lines[0], 'the loop moved'
    c = at[0]
    depth, end = 0, None
    for k in range(c + 1, len(lines)):
        depth += sum(lines[k].count(ch) for ch in '({[') - sum(lines[k].count(ch) for ch in ')}]')
        if depth == 0:
            end = k
            break
    assert end is not None, 'the statement after the comment does not close'
    kept = lines[:c] + [re.sub(r'//\s*', '', lines[c], count=1)] + lines[end + 1:]
    body = '\n'.join(kept)
    assert body.count('{') == body.count('}') and body.count('(') == body.count(')'), 'unbalanced cut'
    return body


def lengths(w):
    return sorted(set(range(13)) | set(range(2 * w - 1, 2 * w + 4)))


def make_cases(rng):
    return [{'window': w, 'values': rng.sample(range(1, 50000), n)} for w in WINDOWS for n in lengths(w)]


def main():
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    src_path = os.path.join(sys.argv[1], *SOURCE)
    loop = cut_loop(src_path)
    cases = make_cases(random.Random(SEED))
    with tempfile.TemporaryDirectory() as tmp:
        src, dst, js = (os.path.join(tmp, n) for n in ('in.json', 'out.json', 'loop.js'))
        json.dump(cases, open(src, 'w'))
        open(js, 'w').write(HARNESS % loop)
        subprocess.check_call(['node', js, src, dst])
        pairs = json.load(open(dst))
    assert len(pairs) == len(cases)
    for c, p in zip(cases, pairs):
        c['pairs'] = p
    fixture = {
        'source': '%s:%d-%d under node' % ('/'.join(SOURCE), FIRST, LAST),
        'windows': list(WINDOWS),
        'cases': cases,
    }
    with open(OUT, 'w') as f:
        json.dump(fixture, f, separators=(',', ':'))
    size = os.path.getsize(OUT)
    print('%s: %d cases, %d pairs, %d bytes' % (OUT, len(cases), sum(len(p) for p in pairs), size))
    assert size < 100 * 1000, 'the fixture must stay under 100 KB'


if __name__ == '__main__':
    sys.exit(main())
