"""Text as UTF-8 (include/bpe.h "text as UTF-8", csrc/bpe_utf8.hip.h): bytes transcoded to UTF-16 units
on the device, in front of the encoder, the corpus ingest and the restore.

Expected values never come from the code under test: they come from bytes.decode('utf-8', 'replace')
(which decodes as Node's Buffer.toString() and the WHATWG decoder do), from rule_decode below, the
per-byte restatement of the rule the kernels implement, and from tests/golden/utf8_cases.json, which
holds what Node itself decoded (tools/gen_utf8_golden.py).
"""
import ctypes
import itertools
import json
import os
import random
import re
import subprocess
import sys

import numpy as np
import pytest

import oracle
from bpe_amd import ROOT, pkg
from golden_util import load_small
from oracle import Corpus, OracleState
from test_restore_text import case_vocab
from test_text_ingest import hist_list, restate

sys.path.insert(0, os.path.join(ROOT, 'tools'))
import gen_utf8_golden as golden  # noqa: E402

T = getattr(pkg, 'UTF8_TILE', 4096)
i64p = ctypes.POINTER(ctypes.c_int64)
EDGE = golden.EDGE
SENTINEL = 0x7EAD


# ---- the rule, restated per byte -------------------------------------------------------------------

def need(b):
    return 2 if 0xC2 <= b <= 0xDF else 3 if 0xE0 <= b <= 0xEF else 4 if 0xF0 <= b <= 0xF4 else 0


def cont(b):
    return 0x80 <= b <= 0xBF


def in_r2(lead, b):
    lo, hi = {0xE0: (0xA0, 0xBF), 0xED: (0x80, 0x9F), 0xF0: (0x90, 0xBF), 0xF4: (0x80, 0x8F)}.get(lead, (0x80, 0xBF))
    return lo <= b <= hi


def rule_decode(t):
    """One text by the local rule: every byte is decided from three bytes on each side of it.
    -> (units, U+FFFD made from ill-formed input)"""
    n = len(t)
    at = lambda i: t[i] if 0 <= i < n else None   # (a position outside the text matches nothing)
    units, replaced = [], 0
    for i, b in enumerate(t):
        p1, p2, p3 = at(i - 1), at(i - 2), at(i - 3)
        if cont(b) and ((p1 is not None and need(p1) >= 2 and in_r2(p1, b)) or
                        (p2 is not None and need(p2) >= 3 and in_r2(p2, p1)) or
                        (p3 is not None and need(p3) == 4 and in_r2(p3, p2) and cont(p1))):
            continue
        k = need(b)
        if b < 0x80:
            units.append(b)
        elif k and at(i + 1) is not None and in_r2(b, at(i + 1)) and \
                all(at(i + j) is not None and cont(at(i + j)) for j in range(2, k)):
            cp = b & (0x1F if k == 2 else 0x0F if k == 3 else 0x07)
            for j in range(1, k):
                cp = (cp << 6) | (t[i + j] & 0x3F)
            if k == 4:
                units += [0xD800 + ((cp - 0x10000) >> 10), 0xDC00 + ((cp - 0x10000) & 0x3FF)]
            else:
                units.append(cp)
        else:
            units.append(0xFFFD)
            replaced += 1
    return units, replaced


def whatwg_decode(t):
    """The WHATWG UTF-8 decoder's state machine (https://encoding.spec.whatwg.org/#utf-8-decoder),
    written out on its own: -> (units, errors)."""
    units, errors = [], 0
    cp = seen = needed = 0
    lower, upper = 0x80, 0xBF

    def emit(c):
        if c > 0xFFFF:
            units.extend([0xD800 + ((c - 0x10000) >> 10), 0xDC00 + ((c - 0x10000) & 0x3FF)])
        else:
            units.append(c)
    i = 0
    while i < len(t):
        b = t[i]
        if needed == 0:
            if b <= 0x7F:
                emit(b)
            elif 0xC2 <= b <= 0xDF:
                needed, cp = 1, b & 0x1F
            elif 0xE0 <= b <= 0xEF:
                lower = 0xA0 if b == 0xE0 else lower
                upper = 0x9F if b == 0xED else upper
                needed, cp = 2, b & 0xF
            elif 0xF0 <= b <= 0xF4:
                lower = 0x90 if b == 0xF0 else lower
                upper = 0x8F if b == 0xF4 else upper
                needed, cp = 3, b & 0x7
            else:
                emit(0xFFFD)
                errors += 1
            i += 1
            continue
        if not lower <= b <= upper:
            cp = needed = seen = 0
            lower, upper = 0x80, 0xBF
            emit(0xFFFD)
            errors += 1
            continue          # (the byte is reprocessed)
        lower, upper = 0x80, 0xBF
        cp = (cp << 6) | (b & 0x3F)
        seen += 1
        i += 1
        if seen == needed:
            emit(cp)
            cp = needed = seen = 0
    if needed:
        emit(0xFFFD)
        errors += 1
    return units, errors


def py_units(t):
    return np.frombuffer(bytes(t).decode('utf-8', 'replace').encode('utf-16-le', 'surrogatepass'), dtype='<u2')


def py_replaced(t):
    """U+FFFD made from ill-formed input: EF BF BD always decodes to U+FFFD (EF is no continuation
    byte, so it always starts a sequence, and BF BD complete it), every other U+FFFD was made.
    (Checked against the state machine's error count on the fixture, below.)"""
    t = bytes(t)
    return t.decode('utf-8', 'replace').count('\ufffd') - t.count(b'\xef\xbf\xbd')


def flat(texts, lead=b''):
    """(uint8 array, int64 offsets) of the texts behind `lead` bytes that belong to no text."""
    off = np.zeros(len(texts) + 1, np.int64)
    np.cumsum([len(t) for t in texts], out=off[1:])
    return np.frombuffer(lead + b''.join(texts), np.uint8), off + len(lead)


def expect(texts):
    none = np.zeros(0, np.uint16)
    parts = [py_units(t) if t else none for t in texts]   # (thousands of empty texts: no call each)
    off = np.zeros(len(texts) + 1, np.int64)
    np.cumsum([len(p) for p in parts], out=off[1:])
    return (np.concatenate(parts) if off[-1] else none), off, sum(py_replaced(t) for t in texts if t)


# ---- CPU ------------------------------------------------------------------------------------------

@pytest.fixture(scope='module')
def fixture():
    with open(os.path.join(ROOT, 'tests', 'golden', 'utf8_cases.json')) as f:
        fx = json.load(f)
    return golden.cases(fx), golden.expected(fx)


def test_restatement_equals_node_and_python_on_every_fixture_case(fixture):
    cases, node = fixture
    assert len(cases) == len(node) == 1 + 27 + 27 ** 2 + 27 ** 3 + 2000 + 500
    assert os.path.getsize(os.path.join(ROOT, 'tests', 'golden', 'utf8_cases.json')) < 300 * 1000
    n_bad = 0
    for t, want in zip(cases, node):
        units, replaced = rule_decode(t)
        assert units == want.tolist() == py_units(t).tolist(), t.hex()
        machine, errors = whatwg_decode(t)
        assert machine == units and errors == replaced == py_replaced(t), t.hex()
        n_bad += replaced > 0
    assert n_bad > 15000   # (most of the range-edge strings are ill-formed)


def test_rule_on_random_bytes():
    rng = random.Random(5)
    for _ in range(3000):
        t = bytes(rng.choice(EDGE) if rng.random() < 0.7 else rng.randrange(256) for _ in range(rng.randint(0, 14)))
        assert rule_decode(t)[0] == py_units(t).tolist(), t.hex()


def test_new_names_are_exported_and_utf8_stats_match_the_header():
    names = ('bpe_encoder_utf8_to_utf16', 'bpe_encoder_utf8_to_utf16_device', 'bpe_encode_utf8_batch',
             'bpe_encode_utf8_batch_device', 'bpe_add_utf8_batch', 'bpe_add_utf8_batch_device',
             'bpe_restore_utf8_batch', 'bpe_restore_utf8_batch_device', 'bpe_encoder_get_utf8_stats',
             'bpe_encoder_reset_utf8_stats', 'bpe_get_utf8_stats', 'bpe_reset_utf8_stats')
    for name in names:
        assert name in pkg.C_API
        assert hasattr(pkg.lib(), name), name
    for name in ('utf8_to_utf16', 'utf8_to_utf16_tensors', 'encode_utf8', 'encode_utf8_tensors', 'utf8_stats',
                 'reset_utf8_stats'):
        assert hasattr(pkg.Encoder, name), name
    for name in ('add_utf8_batch', 'add_utf8_tensors', 'restore_utf8_batch', 'restore_utf8_tensors', 'utf8_stats',
                 'reset_utf8_stats'):
        assert hasattr(pkg.Engine, name), name
    src = open(os.path.join(ROOT, 'include', 'bpe.h')).read()
    body = re.search(r'typedef struct \{([^}]*)\} bpe_utf8_stats;', src).group(1)
    fields = re.findall(r'^\s*(int64_t|double)\s+(\w+);', body, re.M)
    assert [f[1] for f in fields] == [f[0] for f in pkg.Utf8Stats._fields_]
    assert [f[1] for f in fields] == ['calls', 'texts', 'bytes', 'units', 'replaced', 'kernel_ms']
    assert ctypes.sizeof(pkg.Utf8Stats) == 48
    assert int(re.search(r'#define BPE_UTF8_TILE (\d+)', src).group(1)) == pkg.UTF8_TILE == 4096
    if pkg.device_count() == 0:
        with pytest.raises(pkg.BpeError, match='no HIP device'):
            pkg.Encoder(0)


# ---- GPU ------------------------------------------------------------------------------------------

def check(enc, texts, lead=b''):
    """The transcode of one batch against Python: units, offsets and the replaced count."""
    data, off = flat(texts, lead)
    want, want_off, want_rep = expect(texts)
    before = enc.utf8_stats()
    got, got_off = enc.utf8_to_utf16(data, off)
    after = enc.utf8_stats()
    assert np.array_equal(got_off, want_off)
    assert got.dtype == np.uint16 and np.array_equal(got, want)
    assert after['replaced'] - before['replaced'] == want_rep
    assert after['units'] - before['units'] == len(want) and after['bytes'] - before['bytes'] == off[-1] - off[0]
    assert after['texts'] - before['texts'] == len(texts) and after['calls'] - before['calls'] == 1


@pytest.fixture(scope='module')
def enc():
    e = pkg.Encoder(0)
    yield e
    e.close()


@pytest.mark.gpu
def test_every_fixture_case_and_every_edge_string_of_length_4_as_texts_of_one_batch(fixture, enc):
    """531 441 + 22 940 texts, 2.2 MB: about a thousand text boundaries in every tile."""
    cases, node = fixture
    four = [bytes(t) for t in itertools.product(EDGE, repeat=4)]
    texts = cases + four
    data, off = flat(texts)
    rep0 = enc.utf8_stats()['replaced']
    got, got_off = enc.utf8_to_utf16(data, off)
    # the fixture's part against Node, all of it against Python
    n_fx = len(cases)
    assert np.array_equal(got[:got_off[n_fx]], np.concatenate(node))
    assert np.array_equal(np.diff(got_off[:n_fx + 1]), [len(u) for u in node])
    want, want_off, want_rep = expect(texts)
    assert np.array_equal(got_off, want_off) and np.array_equal(got, want)
    assert enc.utf8_stats()['replaced'] - rep0 == want_rep
    assert len(texts) == 27 ** 4 + n_fx


SEQS = [bytes.fromhex(h) for h in (
    'c2a9', 'e282ac', 'f09f9880',                     # well-formed: 2, 3 and 4 bytes
    'c2', 'e282', 'e2', 'f09f98', 'f09f', 'f0',       # their truncations
    'e09f80', 'eda080', 'f08f8080', 'f4908080')]      # second-byte range breaks


def edge_blocks(mis=0):
    """One block of 2 * T bytes per (sequence, byte j of it): ASCII but for the sequence, placed so
    that its byte j is byte 0 of the block's second tile (blocks keep the tiles' phase) when the
    batch's first byte sits `mis` bytes past a 16-B address: the tiles are cut at 16-B addresses, so
    that tile starts at the block's byte T - mis.  Truncated sequences are followed by 'z', so the
    truncation shows."""
    blocks = []
    for s in SEQS:
        for j in range(len(s)):
            b = bytearray(b'a' * (2 * T))
            at = T - mis - j
            b[at:at + len(s)] = s
            b[at + len(s)] = ord('z')
            blocks.append(bytes(b))
    return blocks


def edge_batches(mis):
    """The three batches of the tile-edge cases for a buffer `mis` bytes past a 16-B address: every
    block one text (the first starts with 98 80, which would complete an F0 9F in front of the
    batch); every block cut at the tile edge, before byte j of its sequence (both halves of a cut
    sequence become U+FFFD); and, for one block of every sequence, 5 000 empty texts at that edge."""
    blocks = edge_blocks(mis)
    blocks[0] = b'\x98\x80' + blocks[0][2:]
    cut = T - mis
    halves = [h for b in blocks for h in (b[:cut], b[cut:])]
    firsts = np.cumsum([0] + [len(s) for s in SEQS[:-1]])          # byte 0 of every sequence ...
    picked = [blocks[i + min(1, len(s) - 1)] for i, s in zip(firsts, SEQS)]   # ... or its byte 1: cut inside
    many = [h for b in picked for h in [b[:cut]] + [b''] * 5000 + [b[cut:]]]
    return blocks, halves, many


@pytest.mark.gpu
@pytest.mark.parametrize('lead', [b'\xf0\x9f', b'bbbbb\xf0\x9f'])
def test_sequences_across_a_tile_edge_host_form(enc, lead):
    """Every byte of every sequence in turn as byte 0 of tile 1, through the host form; the batch is a
    slice of a larger buffer (off[0] = len(lead)) whose leading bytes F0 9F must not leak in; then with
    a text boundary at the tile edge and with 5 000 empty texts there.  The host form stages the bytes
    at a 16-B address, so the kernels see no misalignment here whatever off[0] is: the sixteen
    misalignments run through the device form (device_form_check)."""
    blocks, halves, many = edge_batches(0)
    for batch in (blocks, halves, many):
        check(enc, batch, lead)
    assert py_units(halves[6]).tolist()[-1] == 0xFFFD and py_units(halves[7]).tolist()[:2] == [0xFFFD, 0xFFFD]


@pytest.mark.gpu
def test_ascii_tiles_and_the_densest_outputs(enc):
    ascii_tile = bytes(0x20 + i % 95 for i in range(T))
    cyr = 'Ж'.encode() * (T // 2)
    # an all-ASCII tile between two non-ASCII tiles
    check(enc, [cyr + ascii_tile + cyr])
    check(enc, [cyr, ascii_tile[:7], ascii_tile[7:], cyr])
    # a tile that is ASCII but for its last byte F0, whose continuation bytes open the next tile
    check(enc, [ascii_tile[:-1] + b'\xf0\x9f\x98\x80' + ascii_tile])
    check(enc, [ascii_tile[:-1] + b'\xf0', b'\x9f\x98\x80' + ascii_tile])
    check(enc, [b'\x80' * 10000, b'\xf0' * 10000, b'\xf0\x9f\x98\x80' * 10000])
    check(enc, [b'\xf0\x9f\x98\x80' * 10000])
    # units equal bytes
    check(enc, [bytes(0x20 + i % 95 for i in range(3 * T + 5))])
    check(enc, [b'', ascii_tile * 2, b''])


def mixed_text(n, seed):
    """n bytes of mixed scripts with 1 % random bytes."""
    rng = np.random.default_rng(seed)
    piece = ('The quick brown fox. Съешь ещё этих мягких булок. 色は匂へど散りぬるを '
             '😀🎉 naïve café \ufeff\ufffd ').encode()
    b = np.frombuffer(piece * (n // len(piece) + 1), np.uint8)[:n].copy()
    hit = rng.random(n) < 0.01
    b[hit] = rng.integers(0, 256, int(hit.sum()), dtype=np.uint8)
    return b.tobytes()


@pytest.mark.gpu
def test_more_tiles_than_one_scan_round(enc):
    n = (pkg.TEXT_SCAN_ROUND + 37) * T + 123            # 8.5 MB
    blob = mixed_text(n, 11)
    rng = np.random.default_rng(12)
    cuts = np.concatenate([[0], np.cumsum(rng.integers(0, 5001, n // 2400))])
    cuts = np.concatenate([cuts[cuts < n], [n]])
    texts = [blob[a:b] for a, b in zip(cuts[:-1], cuts[1:])]
    assert (n + T - 1) // T > pkg.TEXT_SCAN_ROUND and max(map(len, texts)) <= 5000 and min(map(len, texts)) == 0
    check(enc, texts)


def raw_transcode(enc, data, off, cap, units=None):
    off = np.ascontiguousarray(off, np.int64)
    out_off = np.full(len(off), -77, np.int64)
    rc = pkg.lib().bpe_encoder_utf8_to_utf16(enc._enc, data.ctypes.data, off.ctypes.data_as(i64p), len(off) - 1,
                                             units.ctypes.data if units is not None else None, cap,
                                             out_off.ctypes.data_as(i64p))
    return rc, out_off


@pytest.mark.gpu
def test_capacity_and_arguments(enc):
    texts = ['añ😀'.encode(), b'', b'\xff\xe2\x82', 'z'.encode() * 5000]
    data, off = flat(texts, b'\xc3')
    want, want_off, _ = expect(texts)
    need_units = len(want)
    # the sizing call
    rc, out_off = raw_transcode(enc, data, off, 0)
    assert rc == pkg.ERR_ARG and np.array_equal(out_off, want_off) and out_off[-1] == need_units
    # one short: offsets written, output untouched
    units = np.full(need_units + 8, SENTINEL, np.uint16)
    rc, out_off = raw_transcode(enc, data, off, need_units - 1, units)
    assert rc == pkg.ERR_ARG and np.array_equal(out_off, want_off) and (units == SENTINEL).all()
    assert 'needs %d units' % need_units in pkg.last_error()
    # exact
    rc, out_off = raw_transcode(enc, data, off, need_units, units)
    assert rc == 0 and np.array_equal(out_off, want_off)
    assert np.array_equal(units[:need_units], want) and (units[need_units:] == SENTINEL).all()
    # bad offsets: nothing written
    for bad in ([1, 4, 3, 5, 6], [-1, 2, 3, 4, 5], [3, 2, 4, 5, 6]):
        units[:] = SENTINEL
        rc, out_off = raw_transcode(enc, data, bad, len(units), units)
        assert rc == pkg.ERR_ARG and (out_off == -77).all() and (units == SENTINEL).all(), bad
    # no text, and only empty texts
    rc, out_off = raw_transcode(enc, data, [5], 0)
    assert rc == 0 and out_off.tolist() == [0]
    rc, out_off = raw_transcode(enc, data, [3, 3, 3, 3], 0)
    assert rc == 0 and out_off.tolist() == [0, 0, 0, 0]
    got, got_off = enc.utf8_to_utf16([b'', b''])
    assert got.size == 0 and got_off.tolist() == [0, 0, 0]


INGEST_A = ['abc aé中😀'.encode(), b'', b'ab\xffc\xe2\x82', 'Ж\U00020000'.encode() + b'\xf0\x9f', b'\x80']
INGEST_B = ['cab 中中😀\U0001F389'.encode(), b'\xc0\xaf', b'', 'новый 字'.encode() * 300, b'\xed\xa0\x80!']


@pytest.mark.gpu
def test_ingest_from_utf8_in_two_calls_and_training():
    """New chars of every width, ill-formed bytes (U+FFFD becomes a char token) and empty texts; the
    second call meets a filled char table.  Against the restatement of core.ts:182-207 over the decoded
    strings and the oracle's merges."""
    e = pkg.Engine(0)
    table, nt, all_samples = None, 0, []
    for batch in (INGEST_A, INGEST_B):
        strs = [t.decode('utf-8', 'replace') for t in batch]
        new, hist, samples, table, nt = restate(strs, table, nt)
        got_new, got_hist = e.add_utf8_batch(batch)
        assert got_new.tolist() == new and e.num_tokens() == nt
        assert got_hist.tolist() == hist_list(hist, nt)
        all_samples += samples
        assert e.samples() == all_samples
        ids, soff = e.read_corpus()
        assert ids.tolist() == [i for smp in all_samples for i in smp]
        assert soff.tolist() == np.cumsum([0] + [len(smp) for smp in all_samples]).tolist()
    assert 0xFFFD in table and 0x20000 in table
    counts = np.bincount(np.concatenate([np.asarray(s, np.int64) for s in all_samples]), minlength=nt)
    assert np.array_equal(e.token_counts(), counts)
    st = e.utf8_stats()
    assert st['calls'] == 2 and st['texts'] == 10 and st['bytes'] == sum(map(len, INGEST_A + INGEST_B))
    assert st['replaced'] == sum(py_replaced(t) for t in INGEST_A + INGEST_B) > 8
    c = Corpus()
    for t in INGEST_A + INGEST_B:
        c.add(t.decode('utf-8', 'replace'))
    ost = OracleState.from_corpus(c)
    assert e.merge_until(0, 2, 50) == ost.merge_until(0, 2, 50)
    assert e.samples() == ost.samples()
    e.close()


@pytest.mark.gpu
def test_ingest_new_cap_too_small_changes_nothing_and_the_retry_succeeds():
    e = pkg.Engine(0)
    e.add_utf8_batch([b'ab'])
    before = (e.corpus_size(), e.num_tokens(), e.samples())
    data, off = flat(['abcd\xe9'.encode(), b'\xff'])
    hist = np.zeros(pkg.MAX_VOCAB, np.int64)

    def raw(new_cap):
        new = np.zeros(8, np.uint32)
        n_new = ctypes.c_int64(-7)
        rc = pkg.lib().bpe_add_utf8_batch(e._ctx, data.ctypes.data, off.ctypes.data_as(i64p), 2, new.ctypes.data,
                                          new_cap, ctypes.byref(n_new), hist.ctypes.data_as(i64p), pkg.MAX_VOCAB)
        return rc, n_new.value, new
    rc, n_new, _ = raw(3)
    assert (rc, n_new) == (pkg.ERR_ARG, 4)
    assert (e.corpus_size(), e.num_tokens(), e.samples()) == before
    assert e.utf8_stats()['calls'] == 2 and e.utf8_stats()['texts'] == 1   # (a failed call counts in calls only)
    rc, n_new, new = raw(4)
    assert (rc, n_new) == (0, 4) and new[:4].tolist() == [ord('c'), ord('d'), 0xE9, 0xFFFD]
    assert e.samples() == before[2] + [[0, 1, 2, 3, 4], [5]]
    e.close()


def golden_case():
    from test_encoder_split import split_ok
    return next(c for c in load_small()
                if len(c['merges']) >= 20 and split_ok(case_vocab(c)[1]) and 'Ω' not in case_vocab(c)[0]
                and 4 <= len(case_vocab(c)[0]) and all(len(ch.encode('utf-16-le', 'surrogatepass')) == 2
                                                       for ch in case_vocab(c)[0])
                and all(not 0xD800 <= ord(ch) < 0xE000 for ch in case_vocab(c)[0]))


@pytest.mark.gpu
@pytest.mark.parametrize('mode', ['replay', 'split'])
def test_encode_and_restore_from_utf8(mode):
    """A golden case's merges and chars.  Its own samples against its reference ids; texts of up to
    64 chars, around BPE_TEXT_TILE and longer than BPE_ENCODE_LDS_TOKENS (a char of no merge planted
    every few thousand chars, so that the split mode finds its cuts) against oracle.encode."""
    case = golden_case()
    chars, merges, len16 = case_vocab(case)
    extra = len(len16)
    rng = np.random.default_rng(25)
    texts_ids = []
    for n in (0, 1, 64, pkg.TEXT_TILE - 1, pkg.TEXT_TILE + 1, pkg.ENCODE_LDS_TOKENS + 301):
        t = rng.integers(0, len(chars), n).astype(np.int32)
        t[np.arange(1000, n, 3000)] = extra
        texts_ids.append(t)
    alphabet = chars + ['Ω']
    texts = [''.join(alphabet[i if i != extra else len(chars)] for i in t).encode('utf-8') for t in texts_ids]
    want = [w.tolist() for w in oracle.encode(texts_ids, merges)]
    table = {ch: i for i, ch in enumerate(chars)}
    table['Ω'] = extra
    enc = pkg.Encoder(0, merges, long_texts=mode)
    enc.set_chars(table)
    got = enc.encode_utf8(texts, kind='ids')
    assert [g.tolist() for g in got] == want
    own = [s.encode('utf-8') for s in case['samples']]
    assert [g.tolist() for g in enc.encode_utf8(own, kind='ids')] == case['final_ids']
    index = list(range(extra + 1))
    enc.set_vector_index(index)
    vals, voff = enc.encode_utf8(*flat(texts), kind='vectors')
    assert np.array_equal(vals, np.concatenate([np.asarray(w, np.int32) for w in want]))
    assert np.array_equal(np.diff(voff), [len(w) for w in want])
    e = pkg.Engine(0)
    e.restore_utf8_batch(enc, texts)
    assert e.samples() == want and e.num_tokens() == extra + 1
    flat_want = np.concatenate([np.asarray(w, np.int64) for w in want])
    assert np.array_equal(e.token_counts(), np.bincount(flat_want, minlength=extra + 1))
    if mode == 'split':
        assert enc.split_stats()['texts_fallback'] == 0
    # one ill-formed byte: U+FFFD is not in the table
    before = e.samples()
    s3, unit = texts[3].decode('utf-8'), 70
    bad = [texts[2], b'', s3[:unit].encode('utf-8') + b'\xe2\x82' + s3[unit:].encode('utf-8')]
    data, off = flat(bad)
    vals = np.full(int(off[-1]), 0x7EADBEEF, np.int32)
    out_off = np.full(len(off), -77, np.int64)
    rc = pkg.lib().bpe_encode_utf8_batch(enc._enc, pkg.ENCODE_IDS, data.ctypes.data, off.ctypes.data_as(i64p), 3,
                                         vals.ctypes.data, vals.size, out_off.ctypes.data_as(i64p))
    assert rc == pkg.ERR_VOCAB and pkg.last_error() == 'unknown token, char: U+FFFD (text 2, unit %d)' % unit
    assert (vals == 0x7EADBEEF).all() and (out_off == -77).all()
    with pytest.raises(pkg.BpeError, match=r'unknown token, char: U\+FFFD \(text 2, unit %d\)' % unit) as ei:
        e.restore_utf8_batch(enc, bad)
    assert ei.value.code == pkg.ERR_VOCAB and e.samples() == before
    # ... and with it there
    table['\ufffd'] = extra + 1
    enc.set_chars(table)
    got = enc.encode_utf8(bad, kind='ids')
    ids3 = [table[ch] for ch in bad[2].decode('utf-8', 'replace')]
    assert got[2].tolist() == oracle.encode([np.asarray(ids3, np.int32)], merges)[0].tolist()
    e.restore_utf8_batch(enc, bad)
    assert e.samples() == before + [g.tolist() for g in got]
    e.close()
    enc.close()


@pytest.mark.gpu
def test_multi_device_context():
    """Two shards on device 0 (reduce='host'): ingest and restore from UTF-8 equal one context's."""
    rng = random.Random(31)
    alphabet = [chr(c) for c in range(0x61, 0x6B)] + ['中', 'Ж', '\U0001F600', '\U00020000']
    texts = [''.join(rng.choice(alphabet) for _ in range(rng.choice([0, 5, 400, 3000]))).encode() for _ in range(30)]
    texts[3] += b'\xff\xf0\x9f'
    enc = pkg.Encoder(0, [(0, 1, 40), (40, 2, 41)])
    one, multi = pkg.Engine(0), pkg.Engine(devices=[0, 0], reduce='host')
    assert multi.shard_count() == 2
    res = [e.add_utf8_batch(texts) for e in (one, multi)]
    assert res[0][0].tolist() == res[1][0].tolist() and res[0][1].tolist() == res[1][1].tolist()
    new, hist, samples, table, nt = restate([t.decode('utf-8', 'replace') for t in texts])
    assert res[1][0].tolist() == new and res[1][1].tolist() == hist_list(hist, nt)
    assert multi.utf8_stats()['replaced'] == one.utf8_stats()['replaced'] == 2
    enc.set_chars(table)
    for e in (one, multi):
        e.restore_utf8_batch(enc, texts[:12])
    assert one.samples() == multi.samples() and len(one.samples()) == 42
    assert np.array_equal(one.token_counts(), multi.token_counts())
    assert one.merge_until(4, 2, 50) == multi.merge_until(4, 2, 50)
    assert one.samples() == multi.samples()
    for x in (one, multi, enc):
        x.close()


@pytest.mark.gpu
def test_stats_sum_over_calls_and_reset():
    enc = pkg.Encoder(0)
    a, b = [b'ab\xff', 'é😀'.encode()], [b'\xe2\x82', b'', b'xyz']
    enc.utf8_to_utf16(a)
    enc.utf8_to_utf16(b)
    st = enc.utf8_stats()
    assert (st['calls'], st['texts'], st['bytes'], st['units'], st['replaced']) == (2, 5, 14, 10, 2)
    assert st['kernel_ms'] > 0
    # a failed call counts in calls only: a cap too small, and an encode of a char no table knows
    data, off = flat(a)
    rc, _ = raw_transcode(enc, data, off, 1, np.zeros(8, np.uint16))
    assert rc == pkg.ERR_ARG
    enc.set_chars({'a': 0})
    with pytest.raises(pkg.BpeError, match='unknown token, char'):
        enc.encode_utf8(a, kind='ids')
    st2 = enc.utf8_stats()
    assert st2['calls'] == 4 and {k: st2[k] for k in ('texts', 'bytes', 'units', 'replaced')} == \
        {k: st[k] for k in ('texts', 'bytes', 'units', 'replaced')}
    enc.reset_utf8_stats()
    assert all(v == 0 for v in enc.utf8_stats().values())
    enc.close()


def device_form_check():
    """The device forms on torch uint8 tensors: the tile-edge cases on views at every byte offset 0..15,
    outputs equal to the host forms, text -> vectors without leaving the device, ingest, restore."""
    import torch
    assert torch.cuda.is_available(), 'torch sees no device'
    enc = pkg.Encoder(0)
    # the tile-edge cases at every misalignment of the byte pointer: the kernels cut tiles at 16-B
    # addresses, so tile 1 starts at the view's byte T - mis, and every byte of every sequence in turn
    # sits there; whole blocks, blocks cut at that edge, and 5 000 empty texts at it; F0 9F in front
    for mis in range(16):
        for batch in edge_batches(mis):
            data, off = flat(batch)
            want, want_off, want_rep = expect(batch)
            buf = torch.zeros(len(data) + 64, dtype=torch.uint8, device='cuda')
            k = 16 + (mis - buf.data_ptr()) % 16
            buf[k - 2], buf[k - 1] = 0xF0, 0x9F
            view = buf[k:k + len(data)]
            view.copy_(torch.from_numpy(data.copy()))
            assert view.data_ptr() % 16 == mis
            rep0 = enc.utf8_stats()['replaced']
            units, uoff = enc.utf8_to_utf16_tensors(view, torch.from_numpy(off).cuda())
            assert np.array_equal(uoff.cpu().numpy(), want_off), (mis, len(batch))
            assert np.array_equal(units.cpu().numpy().view(np.uint16), want), (mis, len(batch))
            assert enc.utf8_stats()['replaced'] - rep0 == want_rep, (mis, len(batch))
    blocks = edge_blocks()[:9] + [mixed_text(3 * T + 77, 3), b'', 'конец'.encode()]
    blocks[0] = b'\x98\x80' + blocks[0][2:]   # (would complete the F0 9F in front of the view)
    data, off = flat(blocks)
    want, want_off, want_rep = expect(blocks)
    for mis in range(16):
        buf = torch.zeros(len(data) + 64, dtype=torch.uint8, device='cuda')
        k = 16 + (mis - buf.data_ptr()) % 16
        buf[k - 2], buf[k - 1] = 0xF0, 0x9F
        view = buf[k:k + len(data)]
        view.copy_(torch.from_numpy(data.copy()))
        assert view.data_ptr() % 16 == mis
        units, uoff = enc.utf8_to_utf16_tensors(view, torch.from_numpy(off).cuda())
        assert units.dtype == torch.int16 and units.is_cuda and uoff.is_cuda
        assert np.array_equal(units.cpu().numpy().view(np.uint16), want), mis
        assert np.array_equal(uoff.cpu().numpy(), want_off), mis
    # offsets into a larger tensor (off[0] != 0) and a units output at an odd unit offset
    big = torch.from_numpy(np.concatenate([np.frombuffer(b'\xf0\x9f\x98', np.uint8), data]).copy()).cuda()
    d_off = torch.from_numpy(off + 3).cuda()
    out = torch.full((len(want) + 9,), 0x7EAD, dtype=torch.int16, device='cuda')
    d_ooff = torch.zeros(len(off), dtype=torch.int64, device='cuda')
    need = ctypes.c_int64()
    torch.cuda.synchronize()
    for cap, rc_want in ((len(want) - 1, pkg.ERR_ARG), (len(want), 0)):
        rc = pkg.lib().bpe_encoder_utf8_to_utf16_device(enc._enc, big.data_ptr(), d_off.data_ptr(), len(blocks),
                                                        out[1:].data_ptr(), cap, d_ooff.data_ptr(), ctypes.byref(need))
        assert rc == rc_want and need.value == len(want)
        assert np.array_equal(d_ooff.cpu().numpy(), want_off)
        got = out.cpu().numpy().view(np.uint16)
        assert got[0] == 0x7EAD and (got[1 + len(want):] == 0x7EAD).all()
        assert (got[1:1 + len(want)] == 0x7EAD).all() if rc else np.array_equal(got[1:1 + len(want)], want)
    # text -> vectors on the device
    strs = [b.decode('utf-8', 'replace') for b in blocks]
    new, hist, samples, table, nt = restate(strs)
    enc.set_chars(table)
    enc.set_vector_index(list(range(nt)))
    host_vals, host_off = enc.encode_utf8(data, off, kind='vectors')
    vals, voff = enc.encode_utf8_tensors(big[3:], torch.from_numpy(off).cuda(), kind='vectors')
    assert vals.is_cuda and voff.is_cuda and vals.dtype == torch.int32
    assert np.array_equal(vals.cpu().numpy(), host_vals) and np.array_equal(voff.cpu().numpy(), host_off)
    assert vals.numel() == host_off[-1] == sum(map(len, samples))
    assert [host_vals[host_off[k]:host_off[k + 1]].tolist() for k in range(len(blocks))] == samples
    # ingest and restore
    host, dev = pkg.Engine(0), pkg.Engine(0)
    r_h = host.add_utf8_batch(data, off)
    r_d = dev.add_utf8_tensors(big, d_off)
    assert r_h[0].tolist() == r_d[0].tolist() == new and r_h[1].tolist() == r_d[1].tolist() == hist_list(hist, nt)
    host.restore_utf8_batch(enc, data, off)
    dev.restore_utf8_tensors(enc, big, d_off)
    assert host.samples() == dev.samples() == samples + samples
    assert dev.utf8_stats()['replaced'] == want_rep
    for x in (host, dev, enc):
        x.close()
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
