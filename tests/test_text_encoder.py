"""The text form of the device encoder (bpe_encode_text_batch, csrc/bpe_text.hip.h around
csrc/bpe_encode.hip's kernels): encodeToVector (core.ts:392-445) for batches of UTF-16 texts,
checked against

  - the reference's own data (tests/golden/small_cases.json: every vector and every final id list
    the reference made from its samples), and
  - `py_encode_text`, the Python restatement: code points of the UTF-16 units, the char table, the
    oracle's in-order replay of the merges (oracle.encode), then the vector index — with the
    reference's error order (the first failing text; inside a text the unknown char first),
    on batches laid out around the front end's tile size and scan round, on every route, on both
    forms (host buffers, device tensors) and on every error the header names.
"""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

import oracle
from bpe_amd import pkg
from golden_util import char_weights, compact_index, load_small, token_table_after
from oracle import Corpus, OracleState

T = pkg.TEXT_TILE
KINDS = ['ids', 'vectors']
SENTINEL = 0x7EADBEEF


# ---- the Python restatement ---------------------------------------------------------------------------

class TextError(Exception):
    """The message bpe_last_error must hold."""


def js_str(s):
    """A Python str as a JS string holds it: through UTF-16 units, so a high surrogate next to a low
    one joins into one code point."""
    return s.encode('utf-16-le', 'surrogatepass').decode('utf-16-le', 'surrogatepass')


def units_of(s):
    return np.frombuffer(s.encode('utf-16-le', 'surrogatepass'), dtype='<u2').astype(np.uint16)


def py_encode_text(texts, table, merges, index=None):
    """texts.map(t => encodeToVector(t)) (index: to_vector_index as a list with -1 for holes), or
    the token ids before the index (index None).  table: str of one code point -> id.  Raises
    TextError with the first failing text's error."""
    ids, bad = [], None
    for k, t in enumerate(texts):
        row, unit = [], 0
        for ch in js_str(t):                                  # core.ts:396 (code points)
            if ch not in table:                               # core.ts:398-401
                bad = (k, 'unknown token, char: U+%04X (text %d, unit %d)' % (ord(ch), k, unit))
                break
            row.append(table[ch])
            unit += 2 if ord(ch) > 0xFFFF else 1
        if bad:
            break
        ids.append(np.asarray(row, np.int32))
    out = [e.tolist() for e in oracle.encode(ids, merges)] if ids else []   # core.ts:404-406
    if index is not None:
        for k, row in enumerate(out):
            for i, v in enumerate(row):                       # core.ts:434-444
                if v >= len(index) or index[v] < 0:
                    raise TextError('unknown token index: %d (text %d, position %d)' % (v, k, i))
                row[i] = int(index[v])
    if bad:
        raise TextError(bad[1])
    return out


def np_chars(units, off):
    """The chars of a flat batch, vectorised: (code point of every char, chars before every text).
    Pinned to py_encode_text's `for ch in js_str(t)` by the CPU test below."""
    base, end = int(off[0]), int(off[-1])
    u = units[base:end].astype(np.int64)
    low, high = (u & 0xFC00) == 0xDC00, (u & 0xFC00) == 0xD800
    cont = np.zeros(len(u), bool)
    cont[1:] = low[1:] & high[:-1]
    rel = np.asarray(off, np.int64) - base
    cont[rel[rel < len(u)]] = False                           # a text's first unit starts a char
    start = ~cont
    nxt = np.zeros(len(u), bool)
    nxt[:-1] = cont[1:]
    lo = np.zeros(len(u), np.int64)
    lo[:-1] = u[1:]
    cp = np.where(nxt, 0x10000 + ((u - 0xD800) << 10) + (lo - 0xDC00), u)[start]
    before = np.concatenate([[0], np.cumsum(start)])
    return cp, before[rel]


def np_encode_text(units, off, table, merges, index=None):
    """py_encode_text on the flat form, for batches with no error: (values, out_off)."""
    cp, id_off = np_chars(units, off)
    lut = np.full(0x110000, -1, np.int32)
    for ch, i in table.items():
        lut[ord(ch)] = i
    ids = lut[cp]
    assert (ids >= 0).all()
    rows = oracle.encode([ids[id_off[k]:id_off[k + 1]] for k in range(len(off) - 1)], merges)
    out_off = np.zeros(len(off), np.int64)
    np.cumsum([len(r) for r in rows], out=out_off[1:])
    vals = np.concatenate(rows).astype(np.int32) if out_off[-1] else np.zeros(0, np.int32)
    if index is not None:
        vals = np.asarray(index, np.int32)[vals]
        assert (vals >= 0).all()
    return vals, out_off


def trained_merges(rng, alphabet, n_samples, sample_len, max_iterations=0, min_weight=2):
    """(a, b, c) merges of a reference-style training run (the oracle's mergeUntil)."""
    samples = [rng.integers(0, alphabet, size=rng.integers(0, sample_len + 1)).astype(np.int32)
               for _ in range(n_samples)]
    c = Corpus()
    for s in samples:
        c.add_ids(s)
    c.chars = list(range(alphabet))
    c.len16 = [1] * alphabet
    st = OracleState.from_corpus(c)
    merges = st.merge_until(None, min_weight, max_iterations)
    return [(a, b, alphabet + k) for k, (a, b, _w) in enumerate(merges)]


# ---- the edge vocabulary and its batches ------------------------------------------------------------

H0, H1, L0, L1 = 0xD800, 0xDBFF, 0xDC00, 0xDFFF
JUNK = 0x1234                                                 # a unit no table here knows


def edge_vocab():
    """BMP chars (U+FFFF among them), six pairs plus U+10FFFF, the four boundary lone surrogates;
    ids are a permutation, 24 random merges (every c a fresh id), an index without holes."""
    chars = [chr(0x61 + i) for i in range(20)] + ['é', '中', '￿']
    chars += [chr(0x1F600 + i) for i in range(6)] + ['\U0010FFFF']
    chars += [chr(H0), chr(H1), chr(L0), chr(L1)]
    rng = np.random.default_rng(17)
    ids = rng.permutation(len(chars))
    table = {c: int(i) for c, i in zip(chars, ids)}
    n = len(chars)
    merges = [(int(rng.integers(0, min(n + k, 12))), int(rng.integers(0, n + k)), n + k) for k in range(24)]
    index = rng.permutation(n + len(merges)).astype(np.int32)
    by_id = [None] * n
    for c, i in table.items():
        by_id[i] = c
    return dict(chars=chars, table=table, merges=merges, index=index, by_id=by_id)


def gen(rng, n, pairs=True, lone=True):
    """n units of chars the edge table knows, with no lone high surrogate right before a low one."""
    safe = [0x61 + i for i in range(20)] + [0xE9, 0x4E2D, 0xFFFF]
    cps = np.asarray(safe + ([0x1F600 + i for i in range(6)] + [0x10FFFF] if pairs else []), np.int64)
    pick = cps[rng.integers(0, len(cps), size=n)]
    big = pick > 0xFFFF
    u = np.repeat(pick, 1 + big)
    second = np.zeros(len(u), bool)
    second[np.cumsum(1 + big) - 1] = big
    v = pick - 0x10000
    u = np.where(second, 0xDC00 + (np.repeat(v, 1 + big) & 0x3FF),
                 np.where(np.repeat(big, 1 + big), 0xD800 + (np.repeat(v, 1 + big) >> 10), u))[:n]
    if n and (u[-1] & 0xFC00) == 0xD800:
        u[-1] = 0x61                                          # (a pair cut by the length)
    if lone and n > 8:
        plain = (u & 0xF800) != 0xD800
        ok = np.zeros(n, bool)
        ok[1:-1] = plain[1:-1] & plain[:-2] & plain[2:]
        at = np.nonzero(ok & (np.arange(n) % 3 == 0))[0]
        at = at[rng.random(len(at)) < 0.2]
        u[at] = np.asarray([H0, H1, L0, L1])[rng.integers(0, 4, size=len(at))]
    return u.astype(np.uint16)


def flat(texts, lead=0):
    """texts (unit arrays) -> (units, off) with `lead` junk units before the first text."""
    off = np.zeros(len(texts) + 1, np.int64)
    np.cumsum([len(t) for t in texts], out=off[1:])
    units = np.concatenate([np.full(lead, JUNK, np.uint16)] + [np.asarray(t, np.uint16) for t in texts])
    return units.astype(np.uint16), off + lead


def edge_texts(rng):
    """The issue's list of shapes (host form: the staged units are 16-B aligned, so flat position p
    is slot p % T of tile p // T)."""
    u16 = lambda *a: np.asarray(a, np.uint16)
    t0 = np.concatenate([gen(rng, T - 1, lone=False), u16(H1, L1), gen(rng, 5)])   # H at slot T - 1
    t1 = np.concatenate([gen(rng, T - 7), u16(H1)])           # ends at flat 2T - 1 with a lone H
    t2 = np.concatenate([u16(L1), gen(rng, 20)])              # starts at flat 2T with a lone L
    texts = [u16(), t0, t1, t2, u16(),
             np.concatenate([gen(rng, 10), u16(0x61, H0)]), np.concatenate([u16(L0, 0x62), gen(rng, 3)]),
             u16(H0, 0xD83D, 0xDE00), u16(0xD83D, 0xDE00, L0), u16(L0, H0),
             np.tile(u16(0xD83D, 0xDE03, H1, L1), 25)]
    assert len(t0) + len(t1) == 2 * T and t0[T - 1] == H1 and t0[T] == L1
    texts += [u16()] * 300
    texts += [gen(rng, T - 1), gen(rng, T), gen(rng, T + 1), gen(rng, 2 * T + 1), u16(), u16()]
    return texts


def make_encoder(v, index=True):
    enc = pkg.Encoder(0, v['merges'])
    enc.set_chars(v['table'])
    if index:
        enc.set_vector_index(v['index'])
    return enc


def check_flat(enc, v, units, off):
    for kind in KINDS:
        index = v['index'] if kind == 'vectors' else None
        want, want_off = np_encode_text(units, off, v['table'], v['merges'], index)
        got, got_off = enc.encode_text_flat(units, off, kind)
        assert got.dtype == np.int32 and np.array_equal(got_off, want_off), kind
        assert np.array_equal(got, want), kind


# ---- 1. the reference's own data --------------------------------------------------------------------

def golden_inputs(case):
    c = Corpus()
    for s in case['samples']:
        c.add(s)
    merges = [tuple(m) for m in case['merges']]
    table = token_table_after(c.chars, char_weights(c.samples, len(c.chars)), merges)
    abc = [(a, b, len(c.chars) + k) for k, (a, b, _w) in enumerate(merges)]
    to_vec = compact_index(table)
    index = [to_vec.get(i, -1) for i in range(len(table))]
    return c, abc, table, index


@pytest.mark.gpu
def test_reference_vectors_and_ids_of_every_small_case():
    enc = pkg.Encoder(0)
    n_vec = n_ids = 0
    try:
        for case in load_small():
            c, abc, table, index = golden_inputs(case)
            if not table:
                continue
            enc.clear()
            if abc:
                enc.add_merges(abc)
            enc.set_chars(c.char_to_index)
            enc.set_vector_index(index)
            good = [(s, v) for s, v in zip(case['samples'], case['vectors']) if isinstance(v, list)]
            got = enc.encode_text([s for s, _v in good], 'vectors')
            for g, (_s, v) in zip(got, good):
                assert g.tolist() == v, case['name']
                n_vec += 1
            got = enc.encode_text(case['samples'], 'ids')
            for g, f in zip(got, case['final_ids']):
                assert g.tolist() == f, case['name']
                n_ids += 1
    finally:
        enc.close()
    assert n_vec > 4300 and n_ids >= n_vec, (n_vec, n_ids)


# ---- 2. shapes where the front end can go wrong -----------------------------------------------------

@pytest.mark.gpu
def test_tile_edges_surrogates_and_empty_texts():
    v = edge_vocab()
    rng = np.random.default_rng(4)
    texts = edge_texts(rng)
    enc = make_encoder(v)
    try:
        for lead in (0, 1, 3, 7):
            units, off = flat(texts, lead)
            assert off[0] == lead
            check_flat(enc, v, units, off)
        # the str form, and the per-char restatement on the same batch
        strs = [pkg.units_to_str(t) for t in texts[:12]]
        for kind in KINDS:
            want = py_encode_text(strs, v['table'], v['merges'], v['index'] if kind == 'vectors' else None)
            assert [g.tolist() for g in enc.encode_text(strs, kind)] == want
        # no texts at all, and only empty texts
        for kind in KINDS:
            got, got_off = enc.encode_text_flat(np.zeros(0, np.uint16), np.asarray([5], np.int64), kind)
            assert got.size == 0 and got_off.tolist() == [0]
            got, got_off = enc.encode_text_flat(np.full(3, JUNK, np.uint16), np.asarray([3, 3, 3], np.int64), kind)
            assert got.size == 0 and got_off.tolist() == [0, 0, 0]
        st = enc.text_stats()
        assert st['calls'] == 14 and st['units_in'] > 8 * T and st['chars'] < st['units_in']
    finally:
        enc.close()


@pytest.mark.gpu
def test_few_texts_and_many_ragged_texts():
    v = edge_vocab()
    rng = np.random.default_rng(5)
    enc = make_encoder(v)
    try:
        few = [gen(rng, int(l)) for l in rng.integers(0, 3 * T, size=40)]
        check_flat(enc, v, *flat(few, 2))
        many = [gen(rng, int(l)) for l in rng.integers(0, 40, size=5000)]
        check_flat(enc, v, *flat(many, 5))
    finally:
        enc.close()


@pytest.mark.gpu
def test_more_tiles_than_one_scan_round():
    """A batch longer than TEXT_SCAN_ROUND x T units: the carry from one round of the tile scan
    into the next decides every later id offset.  The texts are cut anywhere in one stream whose
    only pair is U+10FFFF (both halves are in the table as lone chars)."""
    v = edge_vocab()
    rng = np.random.default_rng(6)
    n = pkg.TEXT_SCAN_ROUND * T + 3 * T + 77
    pick = np.asarray([0x61, 0x62, 0x63, 0xE9, 0xFFFF, H1, L1], np.uint16)
    units = pick[rng.integers(0, len(pick), size=n)]
    cap = pkg.ENCODE_LDS_TOKENS
    lens = rng.integers(cap - 3000, cap + 1, size=n // (cap - 3000) + 1)
    off = np.minimum(np.concatenate([[0], np.cumsum(lens)]), n).astype(np.int64)
    off = off[:int(np.argmax(off == n)) + 1]
    assert off[-1] == n and len(off) - 1 > 256 and (np.diff(off) <= cap).all()
    enc = make_encoder(v)
    try:
        enc.reset_stats()
        check_flat(enc, v, units, off)
        assert enc.stats()['texts_replay'] == 0
    finally:
        enc.close()


@pytest.mark.gpu
def test_pack_choice_at_its_edges():
    """One workgroup packs a call of up to 1024 texts and 2^18 units; past either, the scan and the
    gather do.  Both kinds on each side of both edges, and a hole of the index in the last text of
    the 1025-text batch (the gather's last wave)."""
    v = edge_vocab()
    rng = np.random.default_rng(12)
    enc = make_encoder(v)
    try:
        batches = [[gen(rng, int(l)) for l in rng.integers(1, 4, size=n)] for n in (1024, 1025)]
        for total in (1 << 18, (1 << 18) + 1):
            lens = rng.integers(3000, 5000, size=64)
            lens[-1] += total - lens.sum()
            assert lens.sum() == total and 0 < lens[-1] <= pkg.ENCODE_LDS_TOKENS
            batches.append([gen(rng, int(l)) for l in lens])
        enc.reset_stats()
        for texts in batches:
            units, off = flat(texts, 1)
            assert len(units) - 1 == sum(len(t) for t in texts)
            check_flat(enc, v, units, off)
        assert enc.stats()['texts_replay'] == 0
        t = v['table']
        inputs = {x for m in v['merges'] for x in m[:2]}
        hc = next(c for c in v['chars'][:23] if t[c] not in inputs)   # (stands alone wherever it is)
        HC = ord(hc)
        hole = v['index'].copy()
        hole[t[hc]] = -1
        enc.set_vector_index(hole)
        texts = [np.where(x == HC, 0x61 if HC != 0x61 else 0x62, x).astype(np.uint16) for x in batches[1]]
        texts[-1] = np.asarray([0x63, HC, 0x63], np.uint16)
        msg = expect_error(enc, v, 'vectors', texts, hole, lead=1)
        assert msg.startswith('unknown token index: %d (text 1024, position ' % t[hc])
    finally:
        enc.close()


# ---- 3. agreement with the id form ------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize('seed', [1, 2])
def test_ids_equal_the_id_form_on_trained_lists(seed):
    rng = np.random.default_rng(seed)
    alphabet = [12, 40][seed - 1]
    merges = trained_merges(rng, alphabet, 40, 300)
    assert len(merges) > 20
    cps = rng.permutation(np.concatenate([np.arange(0x400, 0x400 + alphabet - 4),
                                          0x1F300 + np.arange(4)]))
    table = {chr(int(c)): i for i, c in enumerate(cps)}
    lengths = [0, 1, 2, 63, 64, 65, 200, 513, 1000, 4097, 9000, pkg.ENCODE_LDS_TOKENS // 2]
    id_texts = [rng.integers(0, alphabet, size=l).astype(np.int32) for l in lengths]
    strs = [''.join(chr(int(cps[i])) for i in t) for t in id_texts]
    enc = pkg.Encoder(0, merges)
    try:
        enc.set_chars(table)
        got = enc.encode_text(strs, 'ids')
        want = enc.encode(id_texts)
        for g, w in zip(got, want):
            assert g.tolist() == w.tolist()
        assert [g.tolist() for g in got] == py_encode_text(strs, table, merges)
    finally:
        enc.close()


# ---- 4. routes ---------------------------------------------------------------------------------------

@pytest.mark.gpu
def test_long_texts_take_the_replay_route():
    """The text form has no path of its own for very large calls (no groups): nothing to test there."""
    v = edge_vocab()
    rng = np.random.default_rng(8)
    cap = pkg.ENCODE_LDS_TOKENS
    enc = make_encoder(v)
    try:
        enc.reset_stats()
        long_bmp = gen(rng, cap + 1, pairs=False)             # 16 385 chars: replay
        check_flat(enc, v, *flat([gen(rng, 30), long_bmp, np.zeros(0, np.uint16), gen(rng, 700)]))
        assert enc.stats()['texts_replay'] == 2               # (once per kind)
        pairs = np.tile(np.asarray([0xD83D, 0xDE01], np.uint16), cap // 2 + 1)   # 16 386 units, 8193 chars
        check_flat(enc, v, *flat([pairs, gen(rng, 9)], 3))
    finally:
        enc.close()


@pytest.mark.gpu
def test_list_the_greedy_cannot_take():
    v = edge_vocab()
    t = v['table']
    a, b, c = t['a'], t['b'], t['c']
    n = len(t)
    v = dict(v, merges=[(a, b, n), (n, a, n + 1), (b, b, a), (a, n, n + 2)])   # c = a is an input of merge 0
    v['index'] = np.arange(n + 3, dtype=np.int32)[::-1].copy()
    rng = np.random.default_rng(9)
    abc = np.asarray([0x61, 0x62, 0x63], np.uint16)
    texts = [abc[rng.integers(0, 3, size=l)] for l in (10, 100, 1000)] + [gen(rng, 50)]
    texts.append(np.asarray([0x62, 0x62, 0x61, 0x62, 0x62, 0x62, 0x61, 0x62], np.uint16))
    enc = make_encoder(v)
    try:
        enc.reset_stats()
        check_flat(enc, v, *flat(texts, 1))
        assert enc.stats()['texts_rank'] == 0
    finally:
        enc.close()


# ---- 5. errors ---------------------------------------------------------------------------------------

def raw_text(enc, kind, units, off, cap=None):
    """bpe_encode_text_batch itself, on outputs pre-filled with marks: (rc, vals, out_off)."""
    units = np.ascontiguousarray(units, np.uint16)
    off = np.ascontiguousarray(off, np.int64)
    if cap is None:
        cap = max(int(off[-1] - off[0]), 0)
    vals = np.full(max(cap, 1), SENTINEL, np.int32)
    out_off = np.full(len(off), -77, np.int64)
    rc = pkg.lib().bpe_encode_text_batch(enc._enc, pkg.Encoder._KINDS[kind], units.ctypes.data,
                                         off.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)), len(off) - 1,
                                         vals.ctypes.data, cap,
                                         out_off.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)))
    return rc, vals, out_off


def expect_error(enc, v, kind, texts, index, lead=0):
    """The call fails with the restatement's message, writes nothing, and a good call follows."""
    strs = [pkg.units_to_str(t) for t in texts]
    with pytest.raises(TextError) as ei:
        py_encode_text(strs, v['table'], v['merges'], index if kind == 'vectors' else None)
    units, off = flat(texts, lead)
    rc, vals, out_off = raw_text(enc, kind, units, off)
    assert rc == pkg.ERR_VOCAB, (rc, pkg.last_error())
    assert pkg.last_error() == str(ei.value)
    assert (vals == SENTINEL).all() and (out_off == -77).all()
    assert [g.tolist() for g in enc.encode_text(['abc'], 'ids')] == py_encode_text(['abc'], v['table'], v['merges'])
    return str(ei.value)


@pytest.mark.gpu
@pytest.mark.parametrize('kind', KINDS)
def test_unknown_chars(kind):
    v = edge_vocab()
    rng = np.random.default_rng(10)
    enc = make_encoder(v)
    try:
        lens = [10, 0, 4 * T, 30, T, 4 * T, 9]

        def batch(marks):
            texts = [gen(rng, l, pairs=False, lone=False) for l in lens]   # (BMP chars around the marks)
            for k, i, units in marks:
                texts[k][i:i + len(units)] = units
            return texts

        z, pair = [0x7A], [0xD83D, 0xDF00]                    # 'z', U+1F700: neither is in the table
        # tile 0 of text 5 and tile 3 of text 2: the earlier flat position wins; then swapped
        msg = expect_error(enc, v, kind, batch([(5, 7, z), (2, 3 * T + 5, pair)]), v['index'])
        assert msg == 'unknown token, char: U+1F700 (text 2, unit %d)' % (3 * T + 5)
        msg = expect_error(enc, v, kind, batch([(2, 7, z), (5, 3 * T + 5, pair)]), v['index'], lead=3)
        assert msg == 'unknown token, char: U+007A (text 2, unit 7)'
        msg = expect_error(enc, v, kind, batch([(5, 3 * T + 5, pair)]), v['index'])
        assert msg == 'unknown token, char: U+1F700 (text 5, unit %d)' % (3 * T + 5)
        # a lone surrogate that only a text boundary makes: the pair is known, its halves are not
        u16 = lambda *a: np.asarray(a, np.uint16)
        msg = expect_error(enc, v, kind, [u16(0x61), u16(0x62, 0xD83D), u16(0xDE00, 0x63)], v['index'])
        assert msg == 'unknown token, char: U+D83D (text 1, unit 1)'
        msg = expect_error(enc, v, kind, [u16(0x61, 0xD83D, 0xDE00), u16(0xDE00, 0x63)], v['index'])
        assert msg == 'unknown token, char: U+DE00 (text 1, unit 0)'
        # an unknown pair whose halves are in the table as lone chars
        msg = expect_error(enc, v, kind, [u16(), u16(0x61, 0x62, H0, L0, 0x63)], v['index'])
        assert msg == 'unknown token, char: U+10000 (text 1, unit 2)'
        # the replay route reports alike
        long_text = gen(rng, pkg.ENCODE_LDS_TOKENS + 5, pairs=False, lone=False)
        long_text[77] = 0x7A
        msg = expect_error(enc, v, kind, [u16(0x61), long_text], v['index'])
        assert msg == 'unknown token, char: U+007A (text 1, unit 77)'
    finally:
        enc.close()


@pytest.mark.gpu
def test_holes_of_the_index_and_the_error_order():
    v = edge_vocab()
    rng = np.random.default_rng(11)
    t = v['table']
    n_tok = len(t) + len(v['merges'])
    u16 = lambda *a: np.asarray(a, np.uint16)
    enc = make_encoder(v)
    try:
        # a hole: a char token no merge takes as an input, so it stands alone wherever it is put
        inputs = {x for m in v['merges'] for x in m[:2]}
        hc = next(c for c in v['chars'][:23] if t[c] not in inputs)
        HC, hid = ord(hc), t[hc]
        hole = v['index'].copy()
        hole[hid] = -1
        enc.set_vector_index(hole)
        texts = [gen(rng, 50, lone=False), gen(rng, 3 * T, lone=False), gen(rng, 20, lone=False)]
        for x in texts:
            x[x == HC] = 0x61 if HC != 0x61 else 0x62
        texts[1][2 * T + 9] = HC
        texts[1][2 * T + 8] = texts[1][2 * T + 10] = 0x63
        texts[2][4] = HC
        texts[2][3] = texts[2][5] = 0x63
        msg = expect_error(enc, v, 'vectors', texts, hole, lead=1)
        assert msg.startswith('unknown token index: %d (text 1, position ' % hid)
        rc, _vals, _off = raw_text(enc, 'ids', *flat(texts))   # ids never meet the index
        assert rc == pkg.BPE_OK
        # an id past the index
        n_chars = len(t)
        short = v['index'][:n_chars - 1].copy()
        enc.set_vector_index(short)
        texts = [units_of(v['by_id'][0]), units_of(v['by_id'][n_chars - 1])]
        msg = expect_error(enc, v, 'vectors', texts, short)
        assert msg == 'unknown token index: %d (text 1, position 0)' % (n_chars - 1)
        # text 0 with a hole, text 1 with an unknown char: the index error; one text with both: the char's
        enc.set_vector_index(hole)
        msg = expect_error(enc, v, 'vectors', [u16(0x63, HC), u16(0x7A)], hole)
        assert msg.startswith('unknown token index: %d (text 0, position ' % hid)
        msg = expect_error(enc, v, 'vectors', [u16(0x61), u16(HC, 0x62, 0x7A)], hole)
        assert msg == 'unknown token, char: U+007A (text 1, unit 2)'
        msg = expect_error(enc, v, 'ids', [u16(0x63, HC), u16(0x7A)], hole)
        assert msg == 'unknown token, char: U+007A (text 1, unit 0)'
        # the same order on the replay route
        long_text = gen(rng, pkg.ENCODE_LDS_TOKENS + 5, pairs=False, lone=False)
        long_text[long_text == HC] = 0x61 if HC != 0x61 else 0x62
        long_text[100] = HC
        msg = expect_error(enc, v, 'vectors', [long_text, u16(0x7A)], hole)
        assert msg.startswith('unknown token index: %d (text 0, position ' % hid)
    finally:
        enc.close()


@pytest.mark.gpu
def test_state_and_argument_errors():
    v = edge_vocab()
    u16 = lambda *a: np.asarray(a, np.uint16)
    enc = pkg.Encoder(0, v['merges'])
    try:
        units, off = flat([u16(0x61, 0x62), u16(0x63)])
        for kind in KINDS:                                    # units without a char table
            rc, vals, out_off = raw_text(enc, kind, units, off)
            assert rc == pkg.ERR_STATE and (vals == SENTINEL).all() and (out_off == -77).all()
        enc.set_chars(v['table'])
        rc, vals, out_off = raw_text(enc, 'vectors', units, off)   # vectors without an index
        assert rc == pkg.ERR_STATE and (vals == SENTINEL).all() and (out_off == -77).all()
        want = py_encode_text(['ab', 'c'], v['table'], v['merges'])
        assert [g.tolist() for g in enc.encode_text(['ab', 'c'], 'ids')] == want
        enc.set_vector_index(v['index'])
        wantv = py_encode_text(['ab', 'c'], v['table'], v['merges'], v['index'])
        assert [g.tolist() for g in enc.encode_text(['ab', 'c'])] == wantv
        # add_merges and clear drop the index; clear keeps the char table
        n_tok = len(v['table']) + len(v['merges'])
        enc.add_merges([(0, 1, n_tok)])
        with pytest.raises(pkg.BpeError) as ei:
            enc.encode_text(['ab'])
        assert ei.value.code == pkg.ERR_STATE
        enc.set_vector_index(v['index'])
        enc.set_vector_index(None)
        with pytest.raises(pkg.BpeError) as ei:
            enc.encode_text(['ab'])
        assert ei.value.code == pkg.ERR_STATE
        enc.set_vector_index(v['index'])
        enc.clear()
        with pytest.raises(pkg.BpeError) as ei:
            enc.encode_text(['ab'])
        assert ei.value.code == pkg.ERR_STATE
        assert [g.tolist() for g in enc.encode_text(['ab', 'c'], 'ids')] == py_encode_text(['ab', 'c'], v['table'], [])
        enc.add_merges(v['merges'])
        enc.set_vector_index(v['index'])
        # vals_cap too small: nothing written; just enough: written
        units, off = flat([units_of('abcabc' * 9), units_of('cab')], 2)
        full, full_off = enc.encode_text_flat(units, off, 'vectors')
        rc, vals, out_off = raw_text(enc, 'vectors', units, off, cap=len(full) - 1)
        assert rc == pkg.ERR_ARG and (vals == SENTINEL).all() and (out_off == -77).all()
        rc, vals, out_off = raw_text(enc, 'vectors', units, off, cap=len(full))
        assert rc == pkg.BPE_OK and np.array_equal(vals[:len(full)], full) and np.array_equal(out_off, full_off)
        # offsets that decrease, or are negative
        for bad in ([0, 5, 4], [-1, 2, 4], [3, 2, 2]):
            rc, vals, out_off = raw_text(enc, 'ids', units, np.asarray(bad, np.int64), cap=8)
            assert rc == pkg.ERR_ARG and (vals == SENTINEL).all() and (out_off == -77).all(), bad
        # set_chars: duplicates, code points and ids out of range leave the old table in force
        for mapping, code in [([(0x61, 1), (0x62, 2), (0x61, 3)], pkg.ERR_ARG),
                              ([(0x1F600, 1), (0x1F600, 2)], pkg.ERR_ARG),
                              ([(0x61, 1), (0x110000, 2)], pkg.ERR_ARG),
                              ([(0x61, 1), (0x62, pkg.MAX_VOCAB)], pkg.ERR_VOCAB),
                              ([(0x61, -1)], pkg.ERR_VOCAB)]:
            cps = np.asarray([m[0] for m in mapping], np.uint32)
            ids = np.asarray([m[1] for m in mapping], np.int32)
            rc = pkg.lib().bpe_encoder_set_chars(enc._enc, cps.ctypes.data,
                                                 ids.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), len(cps))
            assert rc == code, mapping
            assert [g.tolist() for g in enc.encode_text(['ab', 'c'])] == wantv
        enc.set_chars({0x61: v['table']['a'], 'b': v['table']['b']})   # int and str keys; replaces the table
        assert [g.tolist() for g in enc.encode_text(['ab'])] == wantv[:1]
        with pytest.raises(pkg.BpeError, match='U\\+0063') as ei:
            enc.encode_text(['ab', 'c'])
        assert ei.value.code == pkg.ERR_VOCAB
        enc.set_chars({})                                     # n == 0 drops it
        with pytest.raises(pkg.BpeError) as ei:
            enc.encode_text(['ab'], 'ids')
        assert ei.value.code == pkg.ERR_STATE
    finally:
        enc.close()


# ---- 6. the device form and the round trip ------------------------------------------------------------

def device_form_check():
    """encode_text_tensors against the host form, at every misalignment of the unit pointer, and
    text -> vectors -> text on the device.  Returns False when torch sees no device."""
    import torch
    if not torch.cuda.is_available():
        return False
    dev = torch.device('cuda', 0)
    v = edge_vocab()
    rng = np.random.default_rng(4)
    texts = edge_texts(rng)
    enc = make_encoder(v)
    dec = pkg.Decoder(0)
    try:
        dec.add_tokens(v['by_id'])
        dec.add_merges(v['merges'])
        dec.set_vector_index(np.argsort(v['index']).astype(np.int32))
        units0, off0 = flat(texts)
        for kind in KINDS:
            want, want_off = enc.encode_text_flat(units0, off0, kind)
            index = v['index'] if kind == 'vectors' else None
            assert np.array_equal(want, np_encode_text(units0, off0, v['table'], v['merges'], index)[0])
            for lead in (0, 1, 3, 7):
                units, off = flat(texts, lead)
                d_units = torch.from_numpy(units.view(np.int16)).to(dev)
                # off[0] = lead on the whole buffer, and a view from `lead` on (an unaligned pointer)
                for du, do in ((d_units, off), (d_units[lead:], off - lead)):
                    vals, out_off = enc.encode_text_tensors(du, torch.from_numpy(do).to(dev), kind)
                    assert vals.dtype == torch.int32 and out_off.dtype == torch.int64 and vals.is_cuda
                    assert np.array_equal(out_off.cpu().numpy(), want_off), (kind, lead)
                    assert np.array_equal(vals.cpu().numpy(), want), (kind, lead)
        # text -> vectors -> text without leaving the device
        for lead in (0, 1):
            units, off = flat(texts, lead)
            d_units = torch.from_numpy(units.view(np.int16)).to(dev)[lead:]
            d_off = torch.from_numpy(off - lead).to(dev)
            vals, out_off = enc.encode_text_tensors(d_units, d_off, 'vectors')
            back, back_off = dec.decode_tensors(vals, out_off, 'vectors')
            assert torch.equal(back, d_units) and torch.equal(back_off, d_off)
        # an unknown char and a hole on the device: nothing written
        units, off = flat(texts)
        bad = units.copy()
        bad[T + 1:T + 6] = [0x61, 0x61, 0x7A, 0x61, 0x61]
        d_vals = torch.full((len(bad),), SENTINEL, dtype=torch.int32, device=dev)
        d_ooff = torch.full((len(off),), -77, dtype=torch.int64, device=dev)
        d_bad, d_off = torch.from_numpy(bad.view(np.int16)).to(dev), torch.from_numpy(off).to(dev)
        need = ctypes.c_int64()
        torch.cuda.synchronize(dev)
        rc = pkg.lib().bpe_encode_text_batch_device(enc._enc, pkg.ENCODE_VECTORS, d_bad.data_ptr(), d_off.data_ptr(),
                                                    len(off) - 1, d_vals.data_ptr(), len(bad), d_ooff.data_ptr(),
                                                    ctypes.byref(need))
        assert rc == pkg.ERR_VOCAB and pkg.last_error() == 'unknown token, char: U+007A (text 1, unit %d)' % (T + 3)
        assert bool((d_vals == SENTINEL).all()) and bool((d_ooff == -77).all())
        empty = enc.encode_text_tensors(torch.zeros(0, dtype=torch.int16, device=dev),
                                        torch.zeros(1, dtype=torch.int64, device=dev), 'vectors')
        assert empty[0].numel() == 0 and empty[1].tolist() == [0]
        # a trained list
        rng = np.random.default_rng(2)
        merges = trained_merges(rng, 12, 40, 300)
        enc2, dec2 = pkg.Encoder(0, merges), pkg.Decoder(0)
        try:
            chars = [chr(0x3B1 + i) for i in range(10)] + ['\U0001F680', '\ud83d']
            enc2.set_chars({c: i for i, c in enumerate(chars)})
            dec2.add_tokens(chars)
            dec2.add_merges(merges)
            perm = rng.permutation(12 + len(merges)).astype(np.int32)
            enc2.set_vector_index(perm)
            dec2.set_vector_index(np.argsort(perm).astype(np.int32))
            rows = [np.concatenate([units_of(chars[i]) for i in rng.integers(0, 12, size=l)] + [np.zeros(0, np.uint16)])
                    for l in (0, 5, 700, 3000, 1, 64)]
            units, off = flat(rows)
            d_units = torch.from_numpy(units.view(np.int16)).to(dev)
            d_off = torch.from_numpy(off).to(dev)
            vals, out_off = enc2.encode_text_tensors(d_units, d_off, 'vectors')
            assert vals.numel() < d_units.numel()
            back, back_off = dec2.decode_tensors(vals, out_off, 'vectors')
            assert torch.equal(back, d_units) and torch.equal(back_off, d_off)
        finally:
            enc2.close()
            dec2.close()
    finally:
        enc.close()
        dec.close()
    return True


@pytest.mark.gpu
def test_device_form_and_round_trip():
    """In a process of its own that imports torch before libbpe loads (PyTorch sees a device only
    when its HIP runtime is the process's first)."""
    pytest.importorskip('torch')
    here = os.path.dirname(os.path.abspath(__file__))
    env = dict(os.environ, PYTHONPATH=os.pathsep.join(
        [here, os.path.join(os.path.dirname(here), 'oracle'), os.environ.get('PYTHONPATH', '')]))
    out = subprocess.run([sys.executable, os.path.abspath(__file__), 'device-form'], env=env,
                         capture_output=True, text=True, timeout=300)
    if out.returncode == 0 and out.stdout.strip().endswith('no device'):
        pytest.skip('torch sees no device')
    assert out.returncode == 0 and out.stdout.strip().endswith('device form ok'), \
        out.stdout[-2000:] + out.stderr[-3000:]


# ---- 7. CPU ------------------------------------------------------------------------------------------

def test_restatement_reproduces_the_reference_vectors():
    """py_encode_text itself against the reference's data, so the yardstick is pinned."""
    n_vec = n_pairs = n_err = 0
    for case in load_small():
        c, abc, table, index = golden_inputs(case)
        if not table:
            continue
        good = [(s, v) for s, v in zip(case['samples'], case['vectors']) if isinstance(v, list)]
        got = py_encode_text([s for s, _v in good], c.char_to_index, abc, index)
        for g, (s, v) in zip(got, good):
            assert g == v, case['name']
            n_vec += 1
            n_pairs += any(ord(ch) > 0xFFFF for ch in s)
        assert py_encode_text(case['samples'], c.char_to_index, abc) == case['final_ids'], case['name']
        for k, (s, v) in enumerate(zip(case['samples'], case['vectors'])):
            if isinstance(v, str):                            # the reference's own unknown-index errors
                with pytest.raises(TextError, match=v.split(': ', 1)[1] + r' \(text 0, '):
                    py_encode_text([s], c.char_to_index, abc, index)
                n_err += 1
    assert n_vec > 4300 and n_pairs > 400, (n_vec, n_pairs, n_err)


def test_vectorised_restatement_equals_the_per_char_one():
    v = edge_vocab()
    rng = np.random.default_rng(4)
    texts = edge_texts(rng)[:20]
    units, off = flat(texts, 3)
    strs = [pkg.units_to_str(t) for t in texts]
    for kind in KINDS:
        index = v['index'] if kind == 'vectors' else None
        vals, out_off = np_encode_text(units, off, v['table'], v['merges'], index)
        want = py_encode_text(strs, v['table'], v['merges'], index)
        assert [vals[out_off[k]:out_off[k + 1]].tolist() for k in range(len(texts))] == want
    # H H L, H L L, L H and the H | L text boundary, char by char
    cp, id_off = np_chars(*flat([np.asarray(t, np.uint16) for t in
                                 ([H0, 0xD83D, 0xDE00], [0xD83D, 0xDE00, L0], [L0, H0], [0x61, H1], [L1])]))
    assert cp.tolist() == [H0, 0x1F600, 0x1F600, L0, L0, H0, 0x61, H1, L1]
    assert id_off.tolist() == [0, 2, 4, 6, 8, 9]


def test_package_exports_the_text_names():
    L = pkg.lib()
    for name in ('bpe_encoder_set_chars', 'bpe_encoder_set_vector_index', 'bpe_encode_text_batch',
                 'bpe_encode_text_batch_device', 'bpe_encoder_get_text_stats', 'bpe_encoder_reset_text_stats'):
        assert name in pkg.C_API and hasattr(L, name)
    assert (pkg.ENCODE_IDS, pkg.ENCODE_VECTORS) == (0, 1)
    assert T == 2048 and pkg.TEXT_SCAN_ROUND == 2048 and ctypes.sizeof(pkg.TextStats) == 56
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'include', 'bpe.h')).read()
    assert '#define BPE_TEXT_TILE %d\n' % T in hdr and '#define BPE_TEXT_SCAN_ROUND %d\n' % pkg.TEXT_SCAN_ROUND in hdr


if __name__ == '__main__' and sys.argv[1:] == ['device-form']:
    import torch  # noqa: F401  (before libbpe loads)
    print('device form ok' if device_form_check() else 'no device')
