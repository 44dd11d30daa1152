"""Text out as UTF-8 (include/bpe.h "text out as UTF-8", csrc/bpe_utf8_out.hip.h): UTF-16 units
transcoded to bytes on the device, behind the decoder and the corpus export.

Expected values never come from the code under test: they come from rule_encode below, the per-unit
restatement of the rule the kernels implement, from str.encode('utf-8', 'surrogatepass') with every
encoded lone surrogate (ED A0-BF xx) replaced by EF BF BD, and from tests/golden/utf8_out_cases.json,
which holds what Node itself encoded (tools/gen_utf8_out_golden.py).
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

from bpe_amd import ROOT, pkg
from golden_util import compact_index, load_small
from oracle import Corpus, OracleState

sys.path.insert(0, os.path.join(ROOT, 'tools'))
import gen_utf8_out_golden as golden  # noqa: E402

T = getattr(pkg, 'UTF16_TILE', 2048)
i64p = ctypes.POINTER(ctypes.c_int64)
EDGE = golden.EDGE
CANARY = 0xA5
HI, LO = 0xD83D, 0xDE00     # U+1F600 as a pair: F0 9F 98 80
FFFD = b'\xef\xbf\xbd'


# ---- the rule, restated per unit -------------------------------------------------------------------

def hi(u):
    return 0xD800 <= u <= 0xDBFF


def lo(u):
    return 0xDC00 <= u <= 0xDFFF


def rule_encode(t):
    """One text by the local rule: every unit is decided from one unit on each side of it.
    -> (bytes, lone surrogates replaced)"""
    out, replaced = bytearray(), 0
    for i, u in enumerate(t):
        if lo(u) and i > 0 and hi(t[i - 1]):
            continue                                  # absorbed
        if u < 0x80:
            out.append(u)
        elif u < 0x800:
            out += bytes([0xC0 | u >> 6, 0x80 | u & 0x3F])
        elif hi(u) and i + 1 < len(t) and lo(t[i + 1]):
            cp = 0x10000 + ((u & 0x3FF) << 10) + (t[i + 1] & 0x3FF)
            out += bytes([0xF0 | cp >> 18, 0x80 | cp >> 12 & 0x3F, 0x80 | cp >> 6 & 0x3F, 0x80 | cp & 0x3F])
        elif hi(u) or lo(u):
            out += FFFD
            replaced += 1
        else:
            out += bytes([0xE0 | u >> 12, 0x80 | u >> 6 & 0x3F, 0x80 | u & 0x3F])
    return bytes(out), replaced


LONE = re.compile(rb'\xed[\xa0-\xbf][\x80-\xbf]')


def py_encode(t):
    """-> (bytes, replaced) through CPython's encoder."""
    raw = pkg.units_to_str(np.asarray(t, np.uint16)).encode('utf-8', 'surrogatepass')
    return LONE.subn(FFFD, raw)


def flat(texts, lead=()):
    """(uint16 array, int64 offsets) of the texts behind `lead` units that belong to no text."""
    off = np.zeros(len(texts) + 1, np.int64)
    np.cumsum([len(t) for t in texts], out=off[1:])
    parts = [np.asarray(lead, np.uint16)] + [np.asarray(t, np.uint16) for t in texts]
    return np.concatenate(parts), off + len(lead)


def expect(texts):
    parts, rep = [], 0
    for t in texts:
        b, r = py_encode(t) if len(t) else (b'', 0)
        parts.append(b)
        rep += r
    off = np.zeros(len(texts) + 1, np.int64)
    np.cumsum([len(p) for p in parts], out=off[1:])
    return np.frombuffer(b''.join(parts), np.uint8), off, rep


@pytest.fixture(scope='module')
def fixture():
    with open(os.path.join(ROOT, 'tests', 'golden', 'utf8_out_cases.json')) as f:
        fx = json.load(f)
    return golden.cases(fx), golden.expected(fx)


# ---- CPU ------------------------------------------------------------------------------------------

def test_restatement_equals_node_and_python(fixture):
    cases, node = fixture
    assert len(cases) == len(node) == 1 + 14 + 14 ** 2 + 14 ** 3 + 400
    assert os.path.getsize(os.path.join(ROOT, 'tests', 'golden', 'utf8_out_cases.json')) < 300 * 1000
    n_rep = 0
    for t, want in zip(cases, node):
        got, rep = rule_encode(t)
        assert got == want, t
        assert (got, rep) == py_encode(t), t
        assert len(got) <= 3 * len(t)
        n_rep += rep > 0
    assert n_rep > 1500
    assert rule_encode([0xD800, 0xD800, 0xDC00])[0] == FFFD + b'\xf0\x90\x80\x80'
    assert rule_encode([0xD800, 0xDC00, 0xDC00])[0] == b'\xf0\x90\x80\x80' + FFFD
    assert rule_encode([0xFEFF, 0x41])[0] == b'\xef\xbb\xbfA'
    rng = random.Random(7)
    for _ in range(3000):
        t = [rng.choice(EDGE) if rng.random() < 0.6 else rng.randrange(0x10000) for _ in range(rng.randint(0, 14))]
        assert rule_encode(t) == py_encode(t), t


def test_new_names_are_exported_and_utf8_stats_match_the_header():
    names = ('bpe_decoder_utf16_to_utf8', 'bpe_decoder_utf16_to_utf8_device', 'bpe_decode_utf8_batch',
             'bpe_decode_utf8_batch_device', 'bpe_export_utf8_batch', 'bpe_export_utf8_batch_device',
             'bpe_decoder_get_utf8_stats', 'bpe_decoder_reset_utf8_stats')
    for name in names:
        assert name in pkg.C_API
        assert hasattr(pkg.lib(), name), name
    for name in ('utf16_to_utf8', 'utf16_to_utf8_tensors', 'decode_utf8_flat', 'decode_utf8', 'decode_utf8_tensors',
                 'utf8_stats', 'reset_utf8_stats'):
        assert hasattr(pkg.Decoder, name), name
    for name in ('export_utf8_flat', 'export_utf8', 'export_utf8_tensors'):
        assert hasattr(pkg.Engine, name), name
    src = open(os.path.join(ROOT, 'include', 'bpe.h')).read()
    body = re.search(r'typedef struct \{([^}]*)\} bpe_utf8_stats;', src).group(1)
    fields = re.findall(r'^\s*(int64_t|double)\s+(\w+);', body, re.M)
    assert [f[1] for f in fields] == [f[0] for f in pkg.Utf8Stats._fields_]
    assert int(re.search(r'#define BPE_UTF16_TILE (\d+)', src).group(1)) == pkg.UTF16_TILE == 2048


def test_the_lane_rule_on_the_host_under_sanitizers(fixture, tmp_path):
    """u16_classify and its helpers, compiled as plain C++ into a stand-alone program with
    -fsanitize=address,undefined, run as a child process over every fixture case as the texts of one
    batch, at three phases of the runs against the batch."""
    cases, node = fixture
    exe = str(tmp_path / 'classify')
    cmd = ['g++', '-std=c++17', '-O1', '-g', '-fsanitize=address,undefined', '-fno-sanitize-recover=all',
           '-static-libasan', '-static-libubsan',
           '-I', os.path.join(ROOT, 'bpe-tokenizer_amd', 'csrc'), '-o', exe,
           os.path.join(ROOT, 'tests', 'utf8_out_classify_main.cc')]
    built = subprocess.run(cmd, capture_output=True, text=True)
    assert built.returncode == 0, built.stderr[-3000:]
    units, off = flat(cases)
    want = np.frombuffer(b''.join(node), np.uint8)
    want_off = np.concatenate([[0], np.cumsum([len(b) for b in node])])
    want_rep = sum(rule_encode(t)[1] for t in cases)
    for mis in (0, 1, 7):
        src, dst = str(tmp_path / 'in.bin'), str(tmp_path / 'out.bin')
        with open(src, 'wb') as f:
            f.write(np.asarray([len(cases), mis], np.int64).tobytes() + off.tobytes() + units.tobytes())
        run = subprocess.run([exe, src, dst], capture_output=True, text=True, timeout=120)
        assert run.returncode == 0 and not run.stderr, run.stderr[-3000:]
        raw = open(dst, 'rb').read()
        head = np.frombuffer(raw[:8 * (len(cases) + 2)], np.int64)
        assert head[0] == want_rep and np.array_equal(head[1:], want_off), mis
        assert np.array_equal(np.frombuffer(raw[8 * (len(cases) + 2):], np.uint8), want), mis


# ---- GPU ------------------------------------------------------------------------------------------

def check(dec, texts, lead=(), want=None):
    """The transcode of one batch against Python: bytes, offsets and the counters."""
    units, off = flat(texts, lead)
    want, want_off, want_rep = want or expect(texts)
    before = dec.utf8_stats()
    got, got_off = dec.utf16_to_utf8(units, off)
    after = dec.utf8_stats()
    assert np.array_equal(got_off, want_off)
    assert got.dtype == np.uint8 and np.array_equal(got, want)
    assert after['replaced'] - before['replaced'] == want_rep
    assert after['bytes'] - before['bytes'] == len(want) and after['units'] - before['units'] == off[-1] - off[0]
    # (the wrapper's sizing call counts in `calls` only, unless there was nothing to write)
    assert after['texts'] - before['texts'] == len(texts)
    assert after['calls'] - before['calls'] == (2 if len(want) else 1)


@pytest.fixture(scope='module')
def dec():
    d = pkg.Decoder(0)
    yield d
    d.close()


@pytest.mark.gpu
def test_every_fixture_case_and_every_edge_string_of_length_3_as_texts_of_one_batch(fixture, dec):
    cases, node = fixture
    three = [list(t) for t in itertools.product(EDGE, repeat=3)]
    texts = cases + three
    units, off = flat(texts)
    rep0 = dec.utf8_stats()['replaced']
    got, got_off = dec.utf16_to_utf8(units, off)
    n_fx = len(cases)
    assert got[:got_off[n_fx]].tobytes() == b''.join(node)
    assert np.array_equal(np.diff(got_off[:n_fx + 1]), [len(b) for b in node])
    ruled = [rule_encode(t) for t in texts]
    assert got.tobytes() == b''.join(r[0] for r in ruled)
    assert np.array_equal(np.diff(got_off), [len(r[0]) for r in ruled]) and got_off[0] == 0
    assert dec.utf8_stats()['replaced'] - rep0 == sum(r[1] for r in ruled)


SEQS = [[HI, LO], [HI], [LO], [HI, HI, LO], [HI, LO, LO], [LO, HI], [0x4E2D, HI, LO], [0xE9, LO]]
LEADS = [[], [0x61], [0xE9], [0x4E2D]]    # leading texts of 0, 1, 2 and 3 bytes: the tiles' outputs start at odd addresses


def edge_blocks(mis=0):
    """One block of 2 * T units per (sequence, unit j of it): ASCII but for the sequence, placed so that
    its unit j is slot 0 of the block's second tile when the batch's first unit sits `mis` units past a
    16-B address (that tile starts at the block's unit T - mis); 'z' follows the sequence."""
    blocks = []
    for s in SEQS:
        for j in range(len(s) + 1):   # (j == len(s): the sequence ends at slot T - 1)
            b = [0x61] * (2 * T)
            at = T - mis - j
            b[at:at + len(s)] = s
            b[at + len(s)] = 0x7A
            blocks.append(b)
    return blocks


def edge_batches(mis):
    """For a buffer `mis` units past a 16-B address: every block one text; every block cut into texts
    at slots T - 1, 0 and 1 of its second tile (a cut between a high and a low surrogate leaves both
    lone); and 3 000 empty texts at the tile edge of a few blocks."""
    blocks = edge_blocks(mis)
    cut = T - mis
    parts = [p for b in blocks for p in (b[:cut - 1], b[cut - 1:cut], b[cut:cut + 1], b[cut + 1:])]
    many = [h for b in blocks[:5] for h in [b[:cut]] + [[]] * 3000 + [b[cut:]]]
    return blocks, parts, many


@pytest.mark.gpu
@pytest.mark.parametrize('lead_text', range(len(LEADS)))
def test_surrogates_around_a_tile_edge_host_form(dec, lead_text):
    """The host form stages the units at a 16-B address (the misalignments run through the device
    form, device_form_check); the batch is a slice of a larger buffer whose unit before off[0] is a high
    surrogate that must not pair with a low one opening the batch."""
    head = ([LEADS[lead_text]] if LEADS[lead_text] else []) + [[LO, 0x62]]
    blocks, parts, many = edge_batches(sum(map(len, head)))   # (the texts in front shift the blocks)
    for batch in (blocks, parts, many):
        check(dec, head + batch, lead=[0x41, HI])
    # (block 1: the pair's high half at slot T - 1, its low half at slot 0; parts 5 and 6 are those units)
    b, r = rule_encode(parts[5] + parts[6])
    assert rule_encode(parts[5])[1] + rule_encode(parts[6])[1] == 2 and r == 0 and b == b'\xf0\x9f\x98\x80'


@pytest.mark.gpu
def test_ascii_tiles_dense_tiles_and_empty_texts(dec):
    ascii_tile = [0x20 + i % 95 for i in range(T)]
    cjk = [0x4E00 + i % 500 for i in range(T)]           # 3 T bytes from one tile
    check(dec, [cjk + ascii_tile + cjk])
    check(dec, [ascii_tile, cjk, ascii_tile[:7], ascii_tile[7:], cjk])
    check(dec, [cjk[:-1] + [HI], [LO] + cjk])            # 3 (T - 1) + 3 bytes, then lone
    check(dec, [cjk[:-1] + [HI, LO] + cjk])              # 3 (T - 1) + 4 bytes from the first tile
    check(dec, [[HI, LO] * 5000, [HI] * 5000, [LO] * 5000, [0x7FF] * 5000])
    check(dec, [[], ascii_tile * 2 + [0x41] * 5, []])
    check(dec, [[], [], [0x41], [], [], [], [0xE9, HI], [], [], [LO], []])
    check(dec, [[]] * 7)
    got, got_off = dec.utf16_to_utf8([])
    assert got.size == 0 and got_off.tolist() == [0]
    got, got_off = dec.utf16_to_utf8(['añ中😀', '', '\ud83d', '\ude00'])
    assert got.tobytes() == 'añ中😀'.encode() + FFFD * 2 and got_off.tolist() == [0, 10, 10, 13, 16]


def mixed_units(n, seed):
    """n units of mixed scripts with 1 % random units (surrogates among them)."""
    rng = np.random.default_rng(seed)
    piece = np.frombuffer(('The quick brown fox. Съешь ещё этих мягких булок. 色は匂へど散りぬるを '
                           '😀🎉 naïve café \ufeff\ufffd ').encode('utf-16-le'), '<u2')
    u = np.tile(piece, n // len(piece) + 1)[:n].copy()
    hit = rng.random(n) < 0.01
    u[hit] = rng.integers(0xD700, 0xE100, int(hit.sum()), dtype=np.uint16)
    return u


@pytest.mark.gpu
def test_more_tiles_than_one_scan_round(dec):
    n = (pkg.TEXT_SCAN_ROUND + 3) * T - 123              # 4.2 M units
    blob = mixed_units(n, 11)
    rng = np.random.default_rng(12)
    cuts = np.concatenate([[0], np.cumsum(rng.integers(0, 9001, n // 4000))])
    cuts = np.concatenate([cuts[cuts < n], [n]])
    cuts = np.sort(np.concatenate([cuts, cuts[::7]]))    # (empty texts among them)
    texts = [blob[a:b] for a, b in zip(cuts[:-1], cuts[1:])]
    assert (n + T - 1) // T > pkg.TEXT_SCAN_ROUND and min(map(len, texts)) == 0
    check(dec, texts)


def raw_transcode(dec, units, off, cap, out=None):
    off = np.ascontiguousarray(off, np.int64)
    out_off = np.full(len(off), -77, np.int64)
    rc = pkg.lib().bpe_decoder_utf16_to_utf8(dec._dec, units.ctypes.data, off.ctypes.data_as(i64p), len(off) - 1,
                                             out.ctypes.data if out is not None else None, cap,
                                             out_off.ctypes.data_as(i64p))
    return rc, out_off


@pytest.mark.gpu
def test_capacity_and_arguments(dec):
    texts = [[0x61, 0xF1, HI, LO], [], [LO, 0x4E2D], [0x7A] * 5000]
    units, off = flat(texts, lead=[HI])     # off[0] == 1; the unit before it is poison
    want, want_off, _ = expect(texts)
    need = len(want)
    rc, out_off = raw_transcode(dec, units, off, 0)
    assert rc == pkg.ERR_ARG and np.array_equal(out_off, want_off) and out_off[-1] == need
    out = np.full(need + 16, CANARY, np.uint8)
    calls0 = dec.utf8_stats()
    rc, out_off = raw_transcode(dec, units, off, need - 1, out)
    assert rc == pkg.ERR_ARG and np.array_equal(out_off, want_off) and (out == CANARY).all()
    assert 'needs %d bytes' % need in pkg.last_error()
    st = dec.utf8_stats()
    assert st['calls'] == calls0['calls'] + 1 and st['texts'] == calls0['texts'] and st['bytes'] == calls0['bytes']
    rc, out_off = raw_transcode(dec, units, off, need, out)
    assert rc == 0 and np.array_equal(out_off, want_off)
    assert np.array_equal(out[:need], want) and (out[need:] == CANARY).all()
    for bad in ([1, 4, 3, 5, 6], [-1, 2, 3, 4, 5], [3, 2, 4, 5, 6]):
        out[:] = CANARY
        rc, out_off = raw_transcode(dec, units, bad, len(out), out)
        assert rc == pkg.ERR_ARG and (out_off == -77).all() and (out == CANARY).all(), bad
    rc, out_off = raw_transcode(dec, units, [5], 0)
    assert rc == 0 and out_off.tolist() == [0]
    rc, out_off = raw_transcode(dec, units, [3, 3, 3, 3], 0)
    assert rc == 0 and out_off.tolist() == [0, 0, 0, 0]


def golden_case():
    return next(c for c in load_small() if len(c['merges']) >= 20 and len(c['samples']) >= 3
                and all(isinstance(v, list) for v in c['vectors'])
                and any(ord(ch) > 0x7F for s in c['samples'] for ch in s))


def case_decoder(case, dec):
    tt = case['token_table']
    n_chars = len(tt) - len(case['merges'])
    dec.clear()
    dec.add_tokens([t[0] for t in tt[:n_chars]])
    dec.add_merges([(a, b, n_chars + i) for i, (a, b, _w) in enumerate(case['merges'])])
    return n_chars


def restated(strs):
    return [rule_encode(np.frombuffer(s.encode('utf-16-le', 'surrogatepass'), '<u2').tolist())[0] for s in strs]


@pytest.mark.gpu
def test_decode_utf8_on_a_golden_vocabulary():
    case = golden_case()
    d = pkg.Decoder(0)
    try:
        case_decoder(case, d)
        ids = case['final_ids'] + [[]]
        assert d.decode_utf8(ids, kind='ids') == restated(d.decode(ids, kind='ids'))
        assert d.decode_utf8(ids, kind='ids')[:-1] == restated(case['samples'])
        with pytest.raises(pkg.BpeError) as ei:     # BPE_ERR_STATE comes back without an index
            d.decode_utf8(case['vectors'], kind='vectors')
        assert ei.value.code == pkg.ERR_STATE
        d.set_vector_index(list(compact_index(case['token_table']).keys()))
        assert d.decode_utf8(case['vectors'], kind='vectors') == restated(d.decode(case['vectors'], kind='vectors'))
        assert d.decode_utf8(case['vectors']) == restated(case['samples'])
        st = d.utf8_stats()
        # an unknown value: the decoder's message, nothing written, only `calls` moves
        n_tok = d.num_tokens()[0]
        vals = np.asarray([0, 1, n_tok, 0], np.int32)
        off = np.asarray([0, 1, 4], np.int64)
        out = np.full(64, CANARY, np.uint8)
        out_off = np.full(3, -77, np.int64)
        rc = pkg.lib().bpe_decode_utf8_batch(d._dec, pkg.DECODE_IDS, vals.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)),
                                             off.ctypes.data_as(i64p), 2, out.ctypes.data, out.size,
                                             out_off.ctypes.data_as(i64p))
        assert rc == pkg.ERR_VOCAB and pkg.last_error() == 'unknown token index: %d (text 1, position 1)' % n_tok
        assert (out == CANARY).all() and (out_off == -77).all()
        with pytest.raises(pkg.BpeError, match=r'unknown vector index: 60000 \(text 0, position 2\)'):
            d.decode_utf8([[0, 0, 60000]], kind='vectors')
        st2 = d.utf8_stats()
        assert st2['calls'] == st['calls'] + 2
        assert {k: st2[k] for k in ('texts', 'units', 'bytes', 'replaced')} == \
            {k: st[k] for k in ('texts', 'units', 'bytes', 'replaced')}
        # pairing is decided on the decoded text: a lone-high token, then a lone-low token
        d.clear()
        d.add_tokens(['\ud83d', '\ude00', 'a'])
        d.add_merges([(2, 0, 3)])      # 'a' + lone high
        assert d.decode_utf8([[0, 1], [1, 0], [3, 1], [0], [1]], kind='ids') == \
            [b'\xf0\x9f\x98\x80', FFFD * 2, b'a\xf0\x9f\x98\x80', FFFD, FFFD]
    finally:
        d.close()


WELL = ['abc aé中😀', '', 'cab 中中😀\U0001F389 ab ab', 'новый 字 ab' * 300, 'Ж\U00020000 cab']
ILL = [b'ab\xffc\xe2\x82', b'\xed\xa0\x80!', b'\xf0\x9f ab', 'ab ab ab'.encode()]


def engine_and_decoder(texts_bytes, merges=12):
    e = pkg.Engine(0)
    e.add_utf8_batch(texts_bytes)
    done = e.merge_until(0, 2, merges)
    c = Corpus()
    for t in texts_bytes:
        c.add(t.decode('utf-8', 'replace'))
    d = pkg.Decoder(0)
    d.add_tokens(c.chars)
    d.add_merges([(a, b, len(c.chars) + k) for k, (a, b, _w) in enumerate(done)])
    return e, d, c, done


@pytest.mark.gpu
def test_export_utf8_after_ingest_from_utf8_and_merges():
    well = [s.encode('utf-8') for s in WELL]
    e, d, c, done = engine_and_decoder(well)
    try:
        assert len(done) == 12
        assert e.export_utf8(d) == well                  # bytes -> corpus -> merges -> bytes
        idx = [3, 0, 3, 1, 4, 4]
        assert e.export_utf8(d, idx) == [well[k] for k in idx]
        assert e.export_utf8(d, []) == []
        out, off = e.export_utf8_flat(d)
        assert out.dtype == np.uint8 and off.tolist() == np.cumsum([0] + [len(b) for b in well]).tolist()
        # an export only reads: the next merges are those of an engine that never exported
        ost = OracleState.from_corpus(c)
        assert ost.merge_until(0, 2, 12) == done
        assert e.merge_until(0, 2, 30) == ost.merge_until(0, 2, 30)
        with pytest.raises(pkg.BpeError, match=r'unknown token index: \d+ \(text \d+, position \d+\)') as ei:
            e.export_utf8(d)                             # (the decoder knows the first 12 merges only)
        assert ei.value.code == pkg.ERR_VOCAB
        with pytest.raises(pkg.BpeError, match='null decoder'):
            e.export_utf8(None)
    finally:
        e.close()
        d.close()
    # ill-formed input: Node's re-encoding of its decoding
    e, d, c, done = engine_and_decoder(ILL, merges=3)
    try:
        assert e.export_utf8(d) == [t.decode('utf-8', 'replace').encode('utf-8') for t in ILL]
        assert e.export_utf8(d)[1] == FFFD * 3 + b'!'
    finally:
        e.close()
        d.close()


@pytest.mark.gpu
def test_multi_device_context():
    """Two shards on device 0 (reduce='host'): the host form equals one context's, the device form is
    refused with nothing written."""
    well = [s.encode('utf-8') for s in WELL] * 3
    one, multi = pkg.Engine(0), pkg.Engine(devices=[0, 0], reduce='host')
    d = pkg.Decoder(0)
    try:
        for e in (one, multi):
            e.add_utf8_batch(well)
        assert multi.shard_count() == 2
        done = one.merge_until(0, 2, 10)
        assert multi.merge_until(0, 2, 10) == done
        c = Corpus()
        for t in well:
            c.add(t.decode('utf-8'))
        d.add_tokens(c.chars)
        d.add_merges([(a, b, len(c.chars) + k) for k, (a, b, _w) in enumerate(done)])
        n = len(well)
        for idx in (None, list(range(n))[::-1], [n - 1, 0, 5, 5, n - 2], []):
            want = well if idx is None else [well[k] for k in idx]
            assert one.export_utf8(d, idx) == want and multi.export_utf8(d, idx) == want, idx
        need = ctypes.c_int64(-7)
        rc = pkg.lib().bpe_export_utf8_batch_device(multi._ctx, d._dec, None, n, None, 0, None, ctypes.byref(need))
        assert rc == pkg.ERR_ARG and need.value == -7 and 'multi-device' in pkg.last_error()
    finally:
        for x in (one, multi, d):
            x.close()


@pytest.mark.gpu
def test_stats_sum_over_calls_and_reset():
    d = pkg.Decoder(0)
    try:
        d.utf16_to_utf8(['ab\ud83d', 'é😀'])
        d.utf16_to_utf8(['\ude00', '', 'xyz中'])
        st = d.utf8_stats()
        # (each of the two calls is a sizing call, which counts in calls only, and the real one)
        assert (st['calls'], st['texts'], st['units'], st['bytes'], st['replaced']) == (4, 5, 11, 20, 2)
        assert st['kernel_ms'] > 0
        d.add_tokens(['a', '\udc00'])
        assert d.decode_utf8([[0, 1, 0]], kind='ids') == [b'a' + FFFD + b'a']
        st2 = d.utf8_stats()
        assert (st2['calls'], st2['texts'], st2['units'], st2['bytes'], st2['replaced']) == (6, 6, 14, 25, 3)
        assert d.stats()['texts'] == 2 and d.stats()['units_out'] == 6   # (the decode's sizing passes are not counted)
        d.reset_utf8_stats()
        assert all(v == 0 for v in d.utf8_stats().values())
    finally:
        d.close()


def device_form_check():
    """The device forms on torch tensors: the tile-edge cases on unit views 0, 1 and 7 units past a
    16-B address behind leading texts of 0..3 bytes, outputs at odd byte addresses, and decode_utf8 and
    export_utf8 equal to their host forms byte for byte."""
    import torch
    assert torch.cuda.is_available(), 'torch sees no device'
    dec = pkg.Decoder(0)
    for mis in (0, 1, 7):
        for lead_text in LEADS:
            head = ([lead_text] if lead_text else []) + [[LO, 0x62]]
            # (the view's misalignment and the texts in front both shift the blocks against the tiles)
            for batch in edge_batches(mis + sum(map(len, head))):
                texts = head + batch
                units, off = flat(texts)
                want, want_off, want_rep = expect(texts)
                buf = torch.zeros(len(units) + 32, dtype=torch.int16, device='cuda')
                k = 8 + (mis - buf.data_ptr() // 2) % 8
                buf[k - 1] = HI - 0x10000          # a high surrogate in front of the view
                view = buf[k:k + len(units)]
                view.copy_(torch.from_numpy(units.view(np.int16).copy()))
                assert (view.data_ptr() // 2) % 8 == mis
                rep0 = dec.utf8_stats()['replaced']
                out, ooff = dec.utf16_to_utf8_tensors(view, torch.from_numpy(off).cuda())
                assert out.dtype == torch.uint8 and out.is_cuda and ooff.is_cuda
                assert np.array_equal(ooff.cpu().numpy(), want_off), (mis, lead_text, len(texts))
                assert np.array_equal(out.cpu().numpy(), want), (mis, lead_text, len(texts))
                assert dec.utf8_stats()['replaced'] - rep0 == want_rep
    # offsets into a larger tensor (off[0] != 0), an output at an odd byte address, one byte short
    texts = edge_blocks()[:6] + [mixed_units(3 * T + 77, 3).tolist(), [], [0x4E2D, HI]]
    units, off = flat(texts, lead=[0x41, 0x42, HI])
    want, want_off, _ = expect(texts)
    big = torch.from_numpy(units.view(np.int16).copy()).cuda()
    d_off = torch.from_numpy(off).cuda()
    out = torch.full((len(want) + 19,), CANARY, dtype=torch.uint8, device='cuda')
    d_ooff = torch.zeros(len(off), dtype=torch.int64, device='cuda')
    need = ctypes.c_int64()
    torch.cuda.synchronize()
    for cap, rc_want in ((len(want) - 1, pkg.ERR_ARG), (len(want), 0)):
        rc = pkg.lib().bpe_decoder_utf16_to_utf8_device(dec._dec, big.data_ptr(), d_off.data_ptr(), len(texts),
                                                        out[3:].data_ptr(), cap, d_ooff.data_ptr(), ctypes.byref(need))
        assert rc == rc_want and need.value == len(want)
        assert np.array_equal(d_ooff.cpu().numpy(), want_off)
        got = out.cpu().numpy()
        assert (got[:3] == CANARY).all() and (got[3 + len(want):] == CANARY).all()
        assert (got[3:3 + len(want)] == CANARY).all() if rc else np.array_equal(got[3:3 + len(want)], want)
    # decode_utf8: vectors -> bytes on the device
    case = golden_case()
    case_decoder(case, dec)
    dec.set_vector_index(list(compact_index(case['token_table']).keys()))
    vecs = case['vectors'] + [[]]
    host, host_off = dec.decode_utf8_flat(np.concatenate([np.asarray(v, np.int32) for v in vecs]),
                                          np.cumsum([0] + [len(v) for v in vecs]))
    d_vals = torch.from_numpy(np.concatenate([np.asarray(v, np.int32) for v in vecs])).cuda()
    d_voff = torch.from_numpy(np.cumsum([0] + [len(v) for v in vecs]).astype(np.int64)).cuda()
    out, ooff = dec.decode_utf8_tensors(d_vals, d_voff)
    assert out.is_cuda and out.dtype == torch.uint8
    assert np.array_equal(out.cpu().numpy(), host) and np.array_equal(ooff.cpu().numpy(), host_off)
    assert host.tobytes() == b''.join(restated(case['samples']))
    dec.close()
    # export_utf8
    well = [s.encode('utf-8') for s in WELL]
    e, d, _c, _done = engine_and_decoder(well)
    for idx in (None, [3, 0, 3, 1]):
        host, host_off = e.export_utf8_flat(d, idx)
        out, ooff = e.export_utf8_tensors(d, idx)
        assert out.is_cuda and out.dtype == torch.uint8
        assert np.array_equal(out.cpu().numpy(), host) and np.array_equal(ooff.cpu().numpy(), host_off)
    assert host.tobytes() == b''.join(well[k] for k in [3, 0, 3, 1])
    e.close()
    d.close()
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
