"""Lines as samples (include/bpe.h "lines as samples", csrc/bpe_lines.hip.h): the corpus helpers
linesToCorpus, linesTrimmedToCorpus and fileContentToCorpus as a device transform in front of the
ingest and the restore.

Expected values never come from the code under test: they come from tests/golden/lines_cases.json,
which holds what Node's helpers in js/core.js made of each input (tools/gen_lines_golden.py), from
rule_split below, the per-unit restatement of the three modes with the 25 units of trim() written out,
and from np_split, the same restatement vectorised in numpy for the large batches (both checked
against the fixture on every case).
"""
import ctypes
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from bpe_amd import ROOT, pkg
from golden_util import load_small

sys.path.insert(0, os.path.join(ROOT, 'tools'))
import gen_lines_golden as golden  # noqa: E402

T = getattr(pkg, 'TEXT_TILE', 2048)
ROUND = getattr(pkg, 'TEXT_SCAN_ROUND', 2048)
i64p = ctypes.POINTER(ctypes.c_int64)
MODES = ('trim', 'keep', 'file')
CR, LF, FS, EOT = 0x0D, 0x0A, 0x1C, 0x04
# what ECMAScript's trim() removes: WhiteSpace and LineTerminator, 25 units
WS = [0x0009, 0x000A, 0x000B, 0x000C, 0x000D, 0x0020, 0x00A0, 0x1680, 0x2000, 0x2001, 0x2002, 0x2003, 0x2004,
      0x2005, 0x2006, 0x2007, 0x2008, 0x2009, 0x200A, 0x2028, 0x2029, 0x202F, 0x205F, 0x3000, 0xFEFF]
WS_SET = frozenset(WS)
SENTINEL = 0x7EAD


# ---- the rule, restated per unit ---------------------------------------------------------------------

def rule_split(t, mode):
    """One text (a list of units) -> the list of its samples (lists of units)."""
    if mode == 'file':
        return [[FS] + list(t) + [EOT]]
    pieces, cur = [], []
    for u in t:
        if u == LF:
            pieces.append(cur)
            cur = []
        else:
            cur.append(u)
    pieces.append(cur)
    out = []
    for p in pieces:
        if mode == 'trim':
            a, b = 0, len(p)
            while a < b and p[a] in WS_SET:
                a += 1
            while b > a and p[b - 1] in WS_SET:
                b -= 1
            p = p[a:b]
        elif p and p[-1] == CR:
            p = p[:-1]
        out.append([CR] + p + [LF])
    return out


def flat(texts, lead=()):
    """(uint16 array, int64 offsets) of the texts behind `lead` units that belong to no text."""
    off = np.zeros(len(texts) + 1, np.int64)
    np.cumsum([len(t) for t in texts], out=off[1:])
    parts = [np.asarray(lead, np.uint16)] + [np.asarray(t, np.uint16) for t in texts]
    return np.concatenate(parts), off + len(lead)


def rule_batch(texts, mode):
    """texts.flatMap(helper) -> (units, offsets) of the samples."""
    samples = [s for t in texts for s in rule_split(list(t), mode)]
    return flat(samples)


def np_split(units, off, mode):
    """The restatement vectorised: the batch units[off[0]:off[-1]] -> (units, offsets) of its samples."""
    off = np.asarray(off, np.int64)
    n = len(off) - 1
    rel = off - off[0]
    u = np.asarray(units, np.uint16)[off[0]:off[-1]] if n else np.zeros(0, np.uint16)
    total = len(u)
    if mode == 'file':
        b, e = rel[:-1].copy(), rel[1:].copy()
        first, last = FS, EOT
    else:
        first, last = CR, LF
        is_lf = u == LF
        lf_pos = np.flatnonzero(is_lf)
        before = np.concatenate([[0], np.cumsum(is_lf)]).astype(np.int64)   # LFs below each position
        n_s = len(lf_pos) + n
        b, e = np.full(n_s, -1, np.int64), np.full(n_s, -1, np.int64)
        b[before[rel[:-1]] + np.arange(n)] = rel[:-1]
        e[before[rel[1:]] + np.arange(n)] = rel[1:]
        idx = np.arange(len(lf_pos)) + np.searchsorted(rel, lf_pos, side='right') - 1
        e[idx] = lf_pos
        b[idx + 1] = lf_pos + 1
        assert (b >= 0).all() and (e >= b).all()
        if mode == 'trim':
            keep = ~np.isin(u, np.asarray(WS, np.uint16))
            pos = np.arange(total, dtype=np.int64)
            nxt = np.concatenate([np.where(keep, pos, total), [total]])
            nxt = np.minimum.accumulate(nxt[::-1])[::-1]                    # first kept position >= i
            prv = np.concatenate([[-1], np.maximum.accumulate(np.where(keep, pos, -1))])   # last kept < i, at [i]
            b2 = np.minimum(nxt[b], e)
            e2 = np.maximum(prv[e] + 1, b2)
            b, e = b2, e2
        else:
            has_cr = np.zeros(len(e), bool)
            nz = e > b
            has_cr[nz] = u[e[nz] - 1] == CR
            e = e - has_cr
    lens = e - b
    out_off = np.concatenate([[0], np.cumsum(lens + 2)]).astype(np.int64)
    out = np.empty(out_off[-1], np.uint16)
    out[out_off[:-1]] = first
    out[out_off[1:] - 1] = last
    sid = np.repeat(np.arange(len(lens)), lens)
    at = np.arange(len(sid)) - np.repeat(np.cumsum(lens) - lens, lens)
    out[out_off[sid] + 1 + at] = u[b[sid] + at]
    return out, out_off


@pytest.fixture(scope='module')
def fixture():
    with open(os.path.join(ROOT, 'tests', 'golden', 'lines_cases.json')) as f:
        fx = json.load(f)
    cases = golden.cases(fx)
    want = {}
    for mode in MODES:
        samples = [s for per_case in golden.expected(fx, mode, cases) for s in per_case]
        want[mode] = flat(samples)
    return cases, want, fx


# ---- CPU ------------------------------------------------------------------------------------------

def test_restatements_equal_node_on_every_fixture_case(fixture):
    cases, want, fx = fixture
    assert len(cases) == sum(15 ** k for k in range(5)) + 1000 + 200 == fx['n_cases']
    assert os.path.getsize(os.path.join(ROOT, 'tests', 'golden', 'lines_cases.json')) < 100 * 1000
    assert len(WS) == len(WS_SET) == 25
    units, off = flat(cases)
    for mode in MODES:
        node = golden.expected(fx, mode, cases)
        for t, w in zip(cases, node):
            assert rule_split(t, mode) == [s.tolist() for s in w], (mode, t)
        got, got_off = np_split(units, off, mode)
        assert np.array_equal(got_off, want[mode][1]) and np.array_equal(got, want[mode][0]), mode
    # Python's strip() is another set: it takes U+001C and U+0085 and leaves U+FEFF
    assert rule_split([0x1C, 0x85, 0x61, 0xFEFF], 'trim') == [[CR, 0x1C, 0x85, 0x61, LF]]
    assert rule_split([], 'trim') == [[CR, LF]] and rule_split([0x61, LF], 'keep') == [[CR, 0x61, LF], [CR, LF]]
    assert rule_split([0x61, CR, CR, LF, CR], 'keep') == [[CR, 0x61, CR, LF], [CR, LF]]


def test_new_names_are_exported_and_lines_stats_match_the_header():
    names = ('bpe_encoder_split_lines', 'bpe_encoder_split_lines_device', 'bpe_add_lines_batch',
             'bpe_add_lines_batch_device', 'bpe_add_lines_utf8_batch', 'bpe_add_lines_utf8_batch_device',
             'bpe_restore_lines_batch', 'bpe_restore_lines_batch_device', 'bpe_restore_lines_utf8_batch',
             'bpe_restore_lines_utf8_batch_device', 'bpe_encoder_get_lines_stats', 'bpe_encoder_reset_lines_stats',
             'bpe_get_lines_stats', 'bpe_reset_lines_stats')
    for name in names:
        assert name in pkg.C_API
        assert hasattr(pkg.lib(), name), name
    for name in ('split_lines', 'split_lines_flat', 'split_lines_tensors', 'lines_stats', 'reset_lines_stats'):
        assert hasattr(pkg.Encoder, name), name
    for name in ('add_lines', 'add_lines_flat', 'add_lines_tensors', 'add_lines_utf8', 'add_lines_utf8_tensors',
                 'restore_lines', 'restore_lines_tensors', 'restore_lines_utf8', 'restore_lines_utf8_tensors',
                 'lines_stats', 'reset_lines_stats'):
        assert hasattr(pkg.Engine, name), name
    assert (pkg.LINES_TRIM, pkg.LINES_KEEP, pkg.LINES_FILE) == (0, 1, 2)
    src = open(os.path.join(ROOT, 'include', 'bpe.h')).read()
    body = re.search(r'typedef struct \{([^}]*)\} bpe_lines_stats;', src).group(1)
    fields = re.findall(r'^\s*(int64_t|double)\s+(\w+);', body, re.M)
    assert [f[1] for f in fields] == [f[0] for f in pkg.LinesStats._fields_]
    for name, value in (('TRIM', 0), ('KEEP', 1), ('FILE', 2)):
        assert int(re.search(r'#define BPE_LINES_%s (\d+)' % name, src).group(1)) == value


def test_argument_errors_that_need_no_device():
    assert [pkg.lines_mode(m) for m in ('trim', 'keep', 'file', 0, 1, 2)] == [0, 1, 2, 0, 1, 2]
    for bad in ('strip', 3, None, 'TRIM'):
        with pytest.raises(pkg.BpeError, match='unknown lines mode') as ei:
            pkg.lines_mode(bad)
        assert ei.value.code == pkg.ERR_ARG
    # the wrappers resolve the mode and check the offsets before they touch an encoder
    with pytest.raises(pkg.BpeError, match='unknown lines mode'):
        pkg.Encoder.split_lines_flat(None, np.zeros(2, np.uint16), [0, 2], 'lines')
    with pytest.raises(pkg.BpeError, match='must not decrease') as ei:
        pkg.Encoder.split_lines_flat(None, np.zeros(4, np.uint16), [0, 3, 2], 'trim')
    assert ei.value.code == pkg.ERR_ARG
    with pytest.raises(pkg.BpeError, match='unknown lines mode'):
        pkg.Engine.add_lines_flat(None, np.zeros(2, np.uint16), [0, 2], 'lines')
    # the C entry points refuse null handles
    ns = ctypes.c_int64()
    assert pkg.lib().bpe_encoder_split_lines(None, 0, None, None, 0, None, 0, None, 0, ctypes.byref(ns)) == pkg.ERR_ARG
    assert pkg.lib().bpe_add_lines_batch(None, 0, None, None, 0, None, 0, ctypes.byref(ns), None, 0) == pkg.ERR_ARG
    assert pkg.lib().bpe_restore_lines_batch(None, None, 0, None, None, 0) == pkg.ERR_ARG
    if pkg.device_count() == 0:
        with pytest.raises(pkg.BpeError, match='no HIP device') as ei:
            pkg.Encoder(0)
        assert ei.value.code == pkg.ERR_HIP
        with pytest.raises(pkg.BpeError, match='no HIP device') as ei:
            pkg.Engine(0).add_lines(['a\nb'])
        assert ei.value.code == pkg.ERR_HIP


def test_the_rule_on_the_host_under_sanitizers(fixture, tmp_path):
    """The rule of csrc/bpe_lines.hip.h, compiled as plain C++ into a stand-alone program with
    -fsanitize=address,undefined, run as a child process over every fixture case as the texts of one
    batch, in each mode at three phases of the tiles against the batch."""
    cases, want, _ = fixture
    exe = str(tmp_path / 'lines_rule')
    cmd = ['g++', '-std=c++17', '-O1', '-g', '-fsanitize=address,undefined', '-fno-sanitize-recover=all',
           '-static-libasan', '-static-libubsan',
           '-I', os.path.join(ROOT, 'bpe-tokenizer_amd', 'csrc'), '-o', exe,
           os.path.join(ROOT, 'tests', 'lines_rule_main.cc')]
    built = subprocess.run(cmd, capture_output=True, text=True)
    assert built.returncode == 0, built.stderr[-3000:]
    units, off = flat(cases)
    for mode_i, mode in enumerate(MODES):
        for mis in (0, 1, 7):
            src, dst = str(tmp_path / 'in.bin'), str(tmp_path / 'out.bin')
            with open(src, 'wb') as f:
                f.write(np.asarray([len(cases), mis, mode_i], np.int64).tobytes() + off.tobytes() + units.tobytes())
            run = subprocess.run([exe, src, dst], capture_output=True, text=True, timeout=120)
            assert run.returncode == 0 and not run.stderr, run.stderr[-3000:]
            raw = open(dst, 'rb').read()
            n_s = int(np.frombuffer(raw[:8], np.int64)[0])
            assert n_s == len(want[mode][1]) - 1, (mode, mis)
            assert np.array_equal(np.frombuffer(raw[8:8 * (n_s + 2)], np.int64), want[mode][1]), (mode, mis)
            assert np.array_equal(np.frombuffer(raw[8 * (n_s + 2):], np.uint16), want[mode][0]), (mode, mis)


# ---- GPU ------------------------------------------------------------------------------------------

@pytest.fixture(scope='module')
def enc():
    e = pkg.Encoder(0)
    yield e
    e.close()


def check(enc, texts, mode, lead=(), want=None):
    """The split of one batch against the restatement, into buffers of exactly the expected sizes with a
    sentinel on both sides of each: units, offsets, the sentinels and the counters."""
    units, off = flat(texts, lead)
    want, want_off = want or rule_batch(texts, mode)
    n_in, n_s, n_u = int(off[-1] - off[0]), len(want_off) - 1, len(want)
    out, out_off = np.full(n_u + 16, SENTINEL, np.uint16), np.full(n_s + 9, -77, np.int64)
    before = enc.lines_stats()
    rc, ns = raw_split(enc, pkg.lines_mode(mode), units if units.size else np.zeros(1, np.uint16), off,
                       out[8:], out_off[4:], n_u, n_s + 1)
    after = enc.lines_stats()
    assert (rc, ns) == (0, n_s), (mode, pkg.last_error())
    assert np.array_equal(out_off[4:5 + n_s], want_off) and np.array_equal(out[8:8 + n_u], want), mode
    assert (out[:8] == SENTINEL).all() and (out[8 + n_u:] == SENTINEL).all(), mode
    assert (out_off[:4] == -77).all() and (out_off[5 + n_s:] == -77).all(), mode
    assert after['calls'] - before['calls'] == 1 and after['texts'] - before['texts'] == len(texts)
    assert after['units_in'] - before['units_in'] == n_in and after['samples'] - before['samples'] == n_s
    assert after['units_out'] - before['units_out'] == n_u
    assert after['trimmed'] - before['trimmed'] == n_in - (n_u - 2 * n_s)


@pytest.mark.gpu
@pytest.mark.parametrize('mode', MODES)
def test_every_fixture_case_as_texts_of_one_batch(fixture, enc, mode):
    cases, want, _ = fixture
    check(enc, cases, mode, want=want[mode])
    check(enc, cases, mode, lead=[0x20, LF, 0x61], want=want[mode])     # off[0] != 0: units in front are never read
    got, got_off = enc.split_lines_flat(*flat(cases), mode)
    assert got.dtype == np.uint16 and np.array_equal(got, want[mode][0]) and np.array_equal(got_off, want[mode][1])
    assert enc.split_lines([], mode) == []
    assert enc.split_lines(['', ''], mode) == (['\x1c\x04'] * 2 if mode == 'file' else ['\r\n'] * 2)
    assert enc.split_lines([' a\r\n\ufeffb \n', '\x1c c\x85'], mode) == {
        'trim': ['\ra\n', '\rb\n', '\r\n', '\r\x1c c\x85\n'],
        'keep': ['\r a\n', '\r\ufeffb \n', '\r\n', '\r\x1c c\x85\n'],
        'file': ['\x1c a\r\n\ufeffb \n\x04', '\x1c\x1c c\x85\x04']}[mode]


def tile_edge_batches(mis=0):
    """Batches whose interesting unit sits at slots 0, 1, T - 1, T and T + 1 of the tiling of a buffer
    `mis` units past a 16-B address (slot s of the batch's first tile is its unit s - mis)."""
    a, sp = 0x61, 0x20
    out = []
    for slot in (0, 1, T - 1, T, T + 1):
        p = slot - mis
        if p < 0:
            continue
        line = [a] * (2 * T + 40)
        lf = list(line)
        lf[p] = LF                                          # LF at the slot
        out.append([lf])
        crlf = list(line)
        crlf[p] = LF
        if p:
            crlf[p - 1] = CR                                # CR at T - 1 with LF at T, and the like
        out.append([crlf, [a, CR]])                         # ... and a text that ends in CR without LF
        out.append([line[:p], line[p:]])                    # a text boundary at the slot
        out.append([[sp] * p, [sp, a, sp] + [sp] * 30])     # ... with whitespace on both sides of it
        out.append([[a] + [sp] * (p + 5) + [CR], [CR] + [sp] * 9 + [a]])
    run = ([sp, 0x3000, 0x09, 0xFEFF, 0xA0] * T)[:2 * T + 5]
    out.append([run + [a] + [LF] + [a] + run + [LF] + run + [LF] + [a]])          # at a start, an end, a whole line
    out.append([[a] + run[:T + 3], run[T + 3:] + [a], run, [a]])                   # a run cut by a text boundary
    out.append([[0x62 + (i % 7) for i in range(3 * T + 1)] + [LF, a]])             # one long line
    out.append([[], [LF], [], [LF, LF], [CR], [CR, LF, CR]] + [[]] * 300)
    # samples whose boundaries in the output fall on 16-B edges - 1, + 0 and + 1 (8 units each way)
    for n0 in (3, 4, 5, 11, 12, 13):
        out.append([[a] * n0 + [LF] + [a] * 6 + [LF] + [a] * 5 + [LF] + [a] * 7 + [LF] + [a] * 14])
    return out


@pytest.mark.gpu
@pytest.mark.parametrize('mode', MODES)
def test_tile_edges_host_form(enc, mode):
    for batch in tile_edge_batches():
        check(enc, batch, mode)
        check(enc, batch, mode, lead=[0x20])


@pytest.mark.gpu
def test_more_tiles_and_more_lines_than_one_scan_round(enc):
    """About 4.2 M units, mostly `a LF` lines: more tiles than one round of the tile scan and far more
    lines than one round of the length scan, with longer lines, whitespace runs and text boundaries
    sprinkled in."""
    rng = np.random.default_rng(11)
    n = ROUND * T + 5 * T + 123
    assert n > 4.2e6
    u = np.full(n, 0x61, np.uint16)
    u[1::2] = LF
    for at in rng.integers(0, n - 5000, 200):
        k = int(rng.integers(3, 4000))
        u[at:at + k] = rng.choice(np.asarray([0x20, 0x61, 0x3000, 0x0D, 0x62], np.uint16), k)
    off = np.unique(np.concatenate([[0, n], rng.integers(0, n, 40), [T * ROUND, T * ROUND + 1]])).astype(np.int64)
    for mode in ('trim', 'keep'):
        want, want_off = np_split(u, off, mode)
        assert len(want_off) - 1 > 2 * ROUND
        got, got_off = enc.split_lines_flat(u, off, mode)
        assert np.array_equal(got_off, want_off), mode
        assert np.array_equal(got, want), mode


def raw_split(enc, mode, units, off, out, out_off, units_cap=None, off_cap=None):
    ns = ctypes.c_int64(-7)
    rc = pkg.lib().bpe_encoder_split_lines(
        enc._enc, mode, units.ctypes.data, off.ctypes.data_as(i64p), len(off) - 1,
        out.ctypes.data if out is not None else None, len(out) if units_cap is None else units_cap,
        out_off.ctypes.data_as(i64p) if out_off is not None else None,
        len(out_off) if off_cap is None else off_cap, ctypes.byref(ns))
    return rc, ns.value


@pytest.mark.gpu
def test_capacity_protocol_host_form(enc):
    texts = [[0x20, 0x61, LF, 0x62, 0x20], [], [LF]]
    units, off = flat(texts)
    want, want_off = rule_batch(texts, 'trim')
    n_s, n_u = len(want_off) - 1, len(want)
    assert (n_s, n_u) == (5, 12)
    assert raw_split(enc, 0, units, off, None, None, 0, 0) == (pkg.ERR_ARG, n_s)           # the sizing call
    assert 'needs %d units and %d offsets' % (n_u, n_s + 1) in pkg.last_error()
    for ucap, ocap, rc_want in ((n_u - 1, n_s + 1, pkg.ERR_ARG), (n_u, n_s, pkg.ERR_ARG), (n_u, n_s + 1, 0)):
        out = np.full(n_u + 16, SENTINEL, np.uint16)
        out_off = np.full(n_s + 9, -77, np.int64)
        before = enc.lines_stats()
        rc, ns = raw_split(enc, 0, units, off, out[8:], out_off[4:], ucap, ocap)
        assert (rc, ns) == (rc_want, n_s)
        after = enc.lines_stats()
        assert after['calls'] == before['calls'] + 1
        if rc:
            assert (out == SENTINEL).all() and (out_off == -77).all()
            assert all(after[k] == before[k] for k in ('texts', 'units_in', 'samples', 'units_out', 'trimmed'))
        else:
            assert np.array_equal(out[8:8 + n_u], want) and np.array_equal(out_off[4:5 + n_s], want_off)
            assert (out[:8] == SENTINEL).all() and (out[8 + n_u:] == SENTINEL).all()
            assert (out_off[:4] == -77).all() and (out_off[5 + n_s:] == -77).all()
    # no text; unknown modes; offsets out of order
    one = np.full(3, -77, np.int64)
    assert raw_split(enc, 0, units, np.zeros(1, np.int64), None, one[1:], 0, 1) == (0, 0)
    assert one.tolist() == [-77, 0, -77]
    for mode in (-1, 3):
        assert raw_split(enc, mode, units, off, np.zeros(64, np.uint16), np.zeros(16, np.int64))[0] == pkg.ERR_ARG
    assert raw_split(enc, 0, units, np.asarray([0, 3, 2], np.int64), np.zeros(64, np.uint16),
                     np.zeros(16, np.int64))[0] == pkg.ERR_ARG
    assert 'must not decrease' in pkg.last_error()


def helper_samples(strs, mode):
    """texts.flatMap(helper) over str, through the restatement."""
    return [pkg.units_to_str(np.asarray(s, np.uint16)) for t in strs for s in rule_split(pkg._units(t).tolist(), mode)]


def same_context(a, b, merges=50):
    assert a.num_tokens() == b.num_tokens() and a.corpus_size() == b.corpus_size()
    ia, sa = a.read_corpus()
    ib, sb = b.read_corpus()
    assert np.array_equal(ia, ib) and np.array_equal(sa, sb)
    assert np.array_equal(a.token_counts(), b.token_counts())
    if merges:
        assert a.merge_until(0, 2, merges) == b.merge_until(0, 2, merges)
        assert a.samples() == b.samples()


def golden_files():
    """A golden case's sample stream joined into files: LF and CR LF ends, some indentation."""
    case = max(load_small(), key=lambda c: len(c['samples']))
    lines = [s for c in load_small() for s in c['samples']] + list(case['samples'])
    files, ends = [], ['\n', '\r\n', ' \n', '\n\t']
    for i in range(0, len(lines), 40):
        files.append(''.join(line + ends[(i + j) % 4] for j, line in enumerate(lines[i:i + 40])))
    return files


MIXED = ['  съешь ещё\u3000\r\n\tэтих мягких булок \n\n', '我能吞下玻璃 而不伤身体\n \U0001F600 x \r', '',
         '\n', 'no line end', '\ufeffbom first\n\x1c kept \x85\n', 'a\r\r\nb\u200b \n' * 50]
ILL_FORMED = [b' ok \xff\n\xe2\x82 \n', b'\xf0\x9f\x98\x80\r\n\xf0\x9f\n', b'', b'\n\xc0\xaf', 'плюс\n'.encode() * 30]


@pytest.mark.gpu
@pytest.mark.parametrize('mode', MODES)
def test_ingest_from_lines_equals_add_text_of_the_helper_samples(mode):
    for texts in (golden_files(), MIXED):
        for form in ('units', 'utf8'):
            want, e = pkg.Engine(0), pkg.Engine(0)
            w_new, w_hist = want.add_text(helper_samples(texts, mode))
            if form == 'units':
                new, hist = e.add_lines(texts, mode)
            else:
                new, hist = e.add_lines_utf8([t.encode('utf-8') for t in texts], mode=mode)
            assert new.tolist() == w_new.tolist() and hist.tolist() == w_hist.tolist(), (mode, form)
            assert new[0] == (FS if mode == 'file' else CR)     # the first char met is token 0
            same_context(e, want)
            e.close()
            want.close()
    # ill-formed bytes: what bytes.decode('utf-8', 'replace') gives, then the helper
    want, e = pkg.Engine(0), pkg.Engine(0)
    res_w = want.add_text(helper_samples([b.decode('utf-8', 'replace') for b in ILL_FORMED], mode))
    res = e.add_lines_utf8(ILL_FORMED, mode=mode)
    assert res[0].tolist() == res_w[0].tolist() and res[1].tolist() == res_w[1].tolist() and 0xFFFD in res[0]
    assert e.utf8_stats()['replaced'] == sum(b.decode('utf-8', 'replace').count('\ufffd') for b in ILL_FORMED) == 5
    same_context(e, want)
    for x in (want, e):
        x.close()


@pytest.mark.gpu
@pytest.mark.parametrize('long_texts', ['replay', 'split'])
def test_restore_from_lines_equals_restore_text_of_the_helper_samples(long_texts):
    texts = MIXED + [('x' * 999 + 'y') * (pkg.ENCODE_LDS_TOKENS // 1000 + 2) + ' \n tail']
    src = pkg.Engine(0)
    new, _ = src.add_text(texts + ['\x1c\x04'])
    table = {int(cp): i for i, cp in enumerate(new.tolist())}
    src.close()
    a, b = table[ord('x')], table[ord(' ')]
    nt = len(table)
    enc = pkg.Encoder(0, [(a, a, nt), (nt, nt, nt + 1), (b, b, nt + 2)], long_texts=long_texts)
    enc.set_chars(table)
    for mode in MODES:
        want, e_units, e_utf8 = pkg.Engine(0), pkg.Engine(0), pkg.Engine(0)
        want.restore_text(enc, helper_samples(texts, mode))
        e_units.restore_lines(enc, texts, mode)
        e_utf8.restore_lines_utf8(enc, [t.encode('utf-8', 'surrogatepass') for t in texts], mode=mode)
        assert want.samples() == e_units.samples() == e_utf8.samples() and len(want.samples()) >= len(texts)
        assert np.array_equal(want.token_counts(), e_units.token_counts())
        assert np.array_equal(want.token_counts(), e_utf8.token_counts())
        for x in (want, e_units, e_utf8):
            x.close()
    enc.close()


@pytest.mark.gpu
def test_failed_calls_change_nothing_and_count_in_calls_only():
    e = pkg.Engine(0)
    e.add_lines(['ab\n ba '])
    state = (e.corpus_size(), e.num_tokens(), e.token_counts().tolist(), e.samples())
    st = e.lines_stats()
    assert (st['calls'], st['texts'], st['units_in'], st['samples'], st['units_out'], st['trimmed']) == (1, 1, 7, 2, 8, 3)
    assert st['kernel_ms'] > 0

    def unchanged():
        return (e.corpus_size(), e.num_tokens(), e.token_counts().tolist(), e.samples()) == state

    # new_cap too small: n_new says what is needed
    units, off = flat([pkg._units(' cd\nef ').tolist()])
    hist = np.zeros(pkg.MAX_VOCAB, np.int64)
    new, n_new = np.zeros(8, np.uint32), ctypes.c_int64(-7)
    rc = pkg.lib().bpe_add_lines_batch(e._ctx, 0, units.ctypes.data, off.ctypes.data_as(i64p), 1, new.ctypes.data, 3,
                                       ctypes.byref(n_new), hist.ctypes.data_as(i64p), pkg.MAX_VOCAB)
    assert (rc, n_new.value) == (pkg.ERR_ARG, 4) and unchanged()
    # a bad offset, an unknown mode
    bad = np.asarray([0, 5, 3], np.int64)
    rc = pkg.lib().bpe_add_lines_batch(e._ctx, 0, units.ctypes.data, bad.ctypes.data_as(i64p), 2, new.ctypes.data, 8,
                                       ctypes.byref(n_new), hist.ctypes.data_as(i64p), pkg.MAX_VOCAB)
    assert rc == pkg.ERR_ARG and 'must not decrease' in pkg.last_error() and unchanged()
    rc = pkg.lib().bpe_add_lines_batch(e._ctx, 7, units.ctypes.data, off.ctypes.data_as(i64p), 1, new.ctypes.data, 8,
                                       ctypes.byref(n_new), hist.ctypes.data_as(i64p), pkg.MAX_VOCAB)
    assert rc == pkg.ERR_ARG and 'lines mode' in pkg.last_error() and unchanged()
    # an unknown char in the restore: its place is in the produced sample (sample 1 is CR b Z a LF)
    enc = pkg.Encoder(0, [(1, 2, 4)])
    enc.set_chars({'\r': 0, 'a': 1, 'b': 2, '\n': 3})
    with pytest.raises(pkg.BpeError, match=r'unknown token, char: .* \(text 1, unit 2\)') as ei:
        e.restore_lines(enc, ['ab\n  bZa \nba'])
    assert ei.value.code == pkg.ERR_VOCAB and unchanged()
    assert enc.lines_stats()['calls'] == 1 and enc.lines_stats()['texts'] == 0
    st2 = e.lines_stats()
    assert st2['calls'] == 4 and all(st2[k] == st[k] for k in ('texts', 'units_in', 'samples', 'units_out', 'trimmed'))
    # ... and good calls after them
    e.restore_lines(enc, ['ab\n  ba \nba'])
    assert e.samples() == state[3] + [[0, 4, 3], [0, 2, 1, 3], [0, 2, 1, 3]]
    assert enc.lines_stats()['samples'] == 3 and enc.lines_stats()['trimmed'] == 5
    e.add_lines(['q'], 'file')
    assert e.lines_stats()['samples'] == 3 and e.lines_stats()['trimmed'] == 3
    e.reset_lines_stats()
    assert all(v == 0 for v in e.lines_stats().values())
    for x in (e, enc):
        x.close()


@pytest.mark.gpu
def test_multi_device_context():
    """Two shards on device 0 (reduce='host'): the ingest from lines equals one context's."""
    texts = [t.encode('utf-8') for t in golden_files() + MIXED]
    one, multi = pkg.Engine(0), pkg.Engine(devices=[0, 0], reduce='host')
    assert multi.shard_count() == 2
    res = [e.add_lines_utf8(texts) for e in (one, multi)]
    assert res[0][0].tolist() == res[1][0].tolist() and res[0][1].tolist() == res[1][1].tolist()
    assert one.samples() == multi.samples()
    assert np.array_equal(one.token_counts(), multi.token_counts())
    assert one.merge_until(0, 2, 50) == multi.merge_until(0, 2, 50)
    assert one.samples() == multi.samples()
    assert multi.lines_stats()['samples'] == one.lines_stats()['samples'] == len(helper_samples(
        [t.decode('utf-8') for t in texts], 'trim'))
    for x in (one, multi):
        x.close()


def device_form_check():
    """The device forms on torch tensors: the fixture and the tile-edge cases on views at unit offsets
    0..7 with off[0] != 0 and sentinels around both outputs; the capacity protocol; ingest and restore."""
    import torch
    assert torch.cuda.is_available(), 'torch sees no device'
    with open(os.path.join(ROOT, 'tests', 'golden', 'lines_cases.json')) as f:
        fx = json.load(f)
    cases = golden.cases(fx)
    enc = pkg.Encoder(0)

    ns, need = ctypes.c_int64(), ctypes.c_int64()

    def run(texts, mode, mis, oph, want=None):
        """One batch whose first unit sits `mis` units past a 16-B address (two units that belong to no
        text in front of it), straight through the C entry point into an output that starts `oph` units
        past a 16-B address; both outputs exactly sized, with sentinels on both sides."""
        units, off = flat(texts, lead=[0x20, LF])
        want, want_off = want or rule_batch(texts, mode)
        n_s, n_u = len(want_off) - 1, len(want)
        buf = torch.zeros(len(units) + 32, dtype=torch.int16, device='cuda')
        k = 8 + (mis - 2 - buf.data_ptr() // 2) % 8
        view = buf[k:k + len(units)]
        view.copy_(torch.from_numpy(units.view(np.int16).copy()))
        d_off = torch.from_numpy(off).cuda()
        out = torch.full((n_u + 32,), SENTINEL, dtype=torch.int16, device='cuda')
        ko = 8 + (oph - out.data_ptr() // 2) % 8
        d_ooff = torch.full((n_s + 9,), -77, dtype=torch.int64, device='cuda')
        assert (view.data_ptr() // 2 + 2) % 8 == mis and (out[ko:].data_ptr() // 2) % 8 == oph
        torch.cuda.synchronize()
        rc = pkg.lib().bpe_encoder_split_lines_device(
            enc._enc, pkg.lines_mode(mode), view.data_ptr(), d_off.data_ptr(), len(texts), out[ko:].data_ptr(), n_u,
            d_ooff[4:].data_ptr(), n_s + 1, ctypes.byref(ns), ctypes.byref(need))
        assert (rc, ns.value, need.value) == (0, n_s, n_u), (mode, mis, oph, pkg.last_error())
        g, go = out.cpu().numpy().view(np.uint16), d_ooff.cpu().numpy()
        assert np.array_equal(g[ko:ko + n_u], want) and np.array_equal(go[4:5 + n_s], want_off), (mode, mis, oph)
        assert (g[:ko] == SENTINEL).all() and (g[ko + n_u:] == SENTINEL).all(), (mode, mis, oph)
        assert (go[:4] == -77).all() and (go[5 + n_s:] == -77).all(), (mode, mis, oph)
        return view, d_off, want, want_off

    for mode in MODES:
        samples = [s for per_case in golden.expected(fx, mode, cases) for s in per_case]
        want = flat(samples)
        for mis in range(8):
            run(cases, mode, mis, (3 * mis + 1) % 8, want)
    for mode in MODES:
        for mis in range(8):
            for i, batch in enumerate(tile_edge_batches(mis)):
                run(batch, mode, mis, (mis + i) % 8)
    # every head length with every tail length of the emit's partial stores: outputs of 2..17 units
    # (one text of 0..15 units, wrapped) at each of the eight output phases
    for oph in range(8):
        for n in range(16):
            run([[0x62 + j for j in range(n)]], 'file', n % 8, oph)
            run([[0x62 + j for j in range(n)]], 'trim', (n + 3) % 8, oph)
    # the wrapper: a sizing call, or the caller's own buffers in one call
    view, d_off, want, want_off = run(tile_edge_batches(5)[3], 'keep', 5, 2)
    got, got_off = enc.split_lines_tensors(view, d_off, 'keep')
    assert got.is_cuda and got_off.is_cuda and got.dtype == torch.int16
    assert np.array_equal(got.cpu().numpy().view(np.uint16), want) and np.array_equal(got_off.cpu().numpy(), want_off)
    mine = (torch.empty(len(want) + 5, dtype=torch.int16, device='cuda'),
            torch.empty(len(want_off) + 2, dtype=torch.int64, device='cuda'))
    got, got_off = enc.split_lines_tensors(view, d_off, 'keep', out=mine[0], out_off=mine[1])
    assert got.data_ptr() == mine[0].data_ptr() and got_off.data_ptr() == mine[1].data_ptr()
    assert np.array_equal(got.cpu().numpy().view(np.uint16), want) and np.array_equal(got_off.cpu().numpy(), want_off)
    # capacities, with sentinels on both sides of both outputs, at an odd unit offset of the output
    view, d_off, want, want_off = run([[0x20, 0x61, LF, 0x62, 0x20], [], [LF]] * 40, 'trim', 3, 1)
    n_s, n_u = len(want_off) - 1, len(want)
    for ucap, ocap, rc_want in ((0, 0, pkg.ERR_ARG), (n_u - 1, n_s + 1, pkg.ERR_ARG), (n_u, n_s, pkg.ERR_ARG),
                                (n_u, n_s + 1, 0)):
        out = torch.full((n_u + 18,), SENTINEL, dtype=torch.int16, device='cuda')
        d_ooff = torch.full((n_s + 9,), -77, dtype=torch.int64, device='cuda')
        torch.cuda.synchronize()
        rc = pkg.lib().bpe_encoder_split_lines_device(
            enc._enc, 0, view.data_ptr(), d_off.data_ptr(), 120,
            out[9:].data_ptr() if ucap else None, ucap, d_ooff[4:].data_ptr() if ocap else None, ocap,
            ctypes.byref(ns), ctypes.byref(need))
        assert (rc, ns.value, need.value) == (rc_want, n_s, n_u)
        g, go = out.cpu().numpy().view(np.uint16), d_ooff.cpu().numpy()
        if rc:
            assert (g == SENTINEL).all() and (go == -77).all()
        else:
            assert np.array_equal(g[9:9 + n_u], want) and (g[:9] == SENTINEL).all() and (g[9 + n_u:] == SENTINEL).all()
            assert np.array_equal(go[4:5 + n_s], want_off) and (go[:4] == -77).all() and (go[5 + n_s:] == -77).all()
    # ingest and restore from tensors equal the host forms
    texts = MIXED + golden_files()[:3]
    units, off = flat([pkg._units(t).tolist() for t in texts], lead=[LF])
    data = np.frombuffer(b'\n' + b''.join(t.encode('utf-8') for t in texts), np.uint8)
    boff = np.concatenate([[0], np.cumsum([len(t.encode('utf-8')) for t in texts])]).astype(np.int64) + 1
    d_units, d_uoff = torch.from_numpy(units.view(np.int16).copy()).cuda(), torch.from_numpy(off).cuda()
    d_bytes, d_boff = torch.from_numpy(data.copy()).cuda(), torch.from_numpy(boff).cuda()
    for mode in MODES:
        host, dev, dev8 = pkg.Engine(0), pkg.Engine(0), pkg.Engine(0)
        r_h = host.add_lines(texts, mode)
        r_d = dev.add_lines_tensors(d_units, d_uoff, mode)
        r_8 = dev8.add_lines_utf8_tensors(d_bytes, d_boff, mode)
        assert r_h[0].tolist() == r_d[0].tolist() == r_8[0].tolist()
        assert r_h[1].tolist() == r_d[1].tolist() == r_8[1].tolist()
        same_context(dev, host, merges=0)
        same_context(dev8, host, merges=0)
        merges = host.merge_until(0, 2, 50)
        assert dev.merge_until(0, 2, 50) == merges and dev8.merge_until(0, 2, 50) == merges and len(merges) == 50
        assert host.samples() == dev.samples() == dev8.samples()
        table = {int(cp): i for i, cp in enumerate(r_h[0].tolist())}
        renc = pkg.Encoder(0, [(0, 1, len(table))])
        renc.set_chars(table)
        for x in (host, dev, dev8):
            x.close()
        host, dev, dev8 = pkg.Engine(0), pkg.Engine(0), pkg.Engine(0)
        host.restore_lines(renc, texts, mode)
        dev.restore_lines_tensors(renc, d_units, d_uoff, mode)
        dev8.restore_lines_utf8_tensors(renc, d_bytes, d_boff, mode)
        same_context(dev, host, merges=0)
        same_context(dev8, host, merges=0)
        for x in (host, dev, dev8, renc):
            x.close()
    enc.close()
    return True


@pytest.mark.gpu
def test_device_forms_equal_the_host_forms():
    """In a process of its own that imports torch before libbpe loads (PyTorch sees a device only
    when its HIP runtime is the process's first)."""
    here = os.path.dirname(os.path.abspath(__file__))
    env = dict(os.environ, PYTHONPATH=os.pathsep.join(
        [here, os.path.join(os.path.dirname(here), 'oracle'), os.environ.get('PYTHONPATH', '')]))
    out = subprocess.run([sys.executable, os.path.abspath(__file__), 'device-form'], env=env,
                         capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and out.stdout.strip().endswith('device form ok'), \
        out.stdout[-2000:] + out.stderr[-3000:]


if __name__ == '__main__' and sys.argv[1:] == ['device-form']:
    import torch  # noqa: F401  (before libbpe loads)
    print('device form ok' if device_form_check() else 'failed')
