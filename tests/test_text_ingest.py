"""Corpus ingest from text on the device (bpe_set_chars / bpe_add_text_batch, include/bpe.h;
csrc/bpe_ingest.hip.h): addToCorpus (core.ts:182-207) for a batch of UTF-16 texts.

Expected values never come from the code under test:
  - restate():    a per-char restatement of core.ts:182-207 over UTF-16 units (Python strings with
                  lone surrogates, encoded with surrogatepass), pinned against every golden case's
                  char tokens and original weights (which the reference produced itself);
  - restate_np(): the same rule in numpy for the large batches, pinned against restate();
  - the golden cases' merges and final ids, and oracle.Corpus / OracleState for the corpus and the
    training that follows.
"""
import ctypes
import os
import random
import re
import subprocess
import sys

import numpy as np
import pytest

from bpe_amd import ROOT, pkg
from golden_util import load_small
from oracle import Corpus, OracleState

TILE = pkg.TEXT_TILE
i64p = ctypes.POINTER(ctypes.c_int64)


def units_of(text):
    return np.frombuffer(text.encode('utf-16-le', 'surrogatepass'), dtype='<u2').astype(np.uint16)


def pack(texts):
    parts = [units_of(t) for t in texts]
    off = np.zeros(len(parts) + 1, np.int64)
    np.cumsum([len(p) for p in parts], out=off[1:])
    units = np.concatenate(parts) if parts and off[-1] else np.zeros(0, np.uint16)
    return units, off


def restate(texts, table=None, nt=0):
    """core.ts:182-207 per char: (new code points in id order, {id: count}, samples, table, nt)."""
    table = dict(table or {})
    new, hist, samples = [], {}, []
    for t in texts:
        u = units_of(t).tolist()
        ids = []
        i = 0
        while i < len(u):
            x = u[i]
            if 0xD800 <= x < 0xDC00 and i + 1 < len(u) and 0xDC00 <= u[i + 1] < 0xE000:
                cp = 0x10000 + ((x - 0xD800) << 10) + (u[i + 1] - 0xDC00)
                i += 2
            else:
                cp = x
                i += 1
            if cp not in table:
                table[cp] = nt
                new.append(cp)
                nt += 1
            ids.append(table[cp])
            hist[table[cp]] = hist.get(table[cp], 0) + 1
        samples.append(ids)
    return new, hist, samples, table, nt


def restate_np(units, off, table=None, nt=0):
    """The same rule over flat units: (new, hist[nt], ids, id_off, table, nt)."""
    off = np.asarray(off, np.int64)
    u = np.asarray(units).astype(np.int64)[off[0]:off[-1]]
    o = off - off[0]
    n = len(u)
    high, low = (u & 0xFC00) == 0xD800, (u & 0xFC00) == 0xDC00
    first_unit = np.zeros(n, bool)
    first_unit[o[:-1][o[:-1] < n]] = True
    cont = np.zeros(n, bool)
    cont[1:] = low[1:] & high[:-1] & ~first_unit[1:]
    starts = np.flatnonzero(~cont)
    pair = np.zeros(n, bool)
    pair[:-1] = cont[1:]
    key = u[starts].copy()
    p = pair[starts]
    key[p] = 0x10000 + ((u[starts[p]] - 0xD800) << 10) + (u[starts[p] + 1] - 0xDC00)
    uniq, first, inv = np.unique(key, return_index=True, return_inverse=True)
    table = dict(table or {})
    new = []
    for j in np.argsort(first, kind='stable'):
        cp = int(uniq[j])
        if cp not in table:
            table[cp] = nt
            new.append(cp)
            nt += 1
    idmap = np.asarray([table[int(c)] for c in uniq], np.int64)
    ids = idmap[inv] if n else np.zeros(0, np.int64)
    hist = np.bincount(ids, minlength=nt).astype(np.int64)
    return new, hist, ids.astype(np.int32), np.searchsorted(starts, o, 'left').astype(np.int64), table, nt


def hist_list(hist, nt):
    return [hist.get(i, 0) for i in range(nt)]


def beyond_latin1(case):
    return any(ord(ch) > 255 for s in case['samples'] for ch in s)


def wide(case):
    """Holds a supplementary char or a lone surrogate."""
    return any(ord(ch) > 0xFFFF or 0xD800 <= ord(ch) < 0xE000 for s in case['samples'] for ch in s)


# ---- CPU ------------------------------------------------------------------------------------------

def test_restatement_reproduces_every_golden_case():
    """The char tokens in order (token_table[i][0]) and their original_weight (token_table[i][2])
    of all 1509 cases; 221 of them hold text beyond latin1."""
    cases = load_small()
    assert len(cases) == 1509
    assert sum(beyond_latin1(c) for c in cases) == 221 == sum(beyond_latin1(c) and wide(c) for c in cases)
    for case in cases:
        new, hist, samples, _, nt = restate(case['samples'])
        n_chars = len(case['token_table']) - len(case['merges'])
        assert nt == n_chars, case['name']
        assert [chr(cp) for cp in new] == [t[0] for t in case['token_table'][:nt]], case['name']
        assert hist_list(hist, nt) == [t[2] for t in case['token_table'][:nt]], case['name']


def test_numpy_restatement_equals_the_per_char_one():
    rng = random.Random(7)
    alphabet = ['a', 'b', 'é', '中', '\U0001F600', '\U00020000', '\ud800', '\udc00', '\udbff', '\udfff']
    for trial in range(300):
        texts = [''.join(rng.choice(alphabet) for _ in range(rng.choice([0, 0, 1, 2, 5, 30])))
                 for _ in range(rng.choice([1, 2, 7]))]
        table = {ord('b'): 0, 0x20000: 1} if trial % 2 else None
        nt0 = 2 if table else 0
        new, hist, samples, tab, nt = restate(texts, table, nt0)
        units, off = pack(texts)
        new2, hist2, ids2, id_off2, tab2, nt2 = restate_np(units, off, table, nt0)
        assert (new2, nt2, tab2) == (new, nt, tab)
        assert hist2.tolist() == hist_list(hist, nt)
        assert [ids2[id_off2[k]:id_off2[k + 1]].tolist() for k in range(len(texts))] == samples


def test_new_names_are_exported_and_ingest_stats_match_the_header():
    for name in ('bpe_set_chars', 'bpe_add_text_batch', 'bpe_add_text_batch_device', 'bpe_get_ingest_stats',
                 'bpe_reset_ingest_stats'):
        assert name in pkg.C_API
        assert hasattr(pkg.lib(), name), name
    for name in ('set_chars', 'add_text', 'add_text_flat', 'add_text_tensors', 'ingest_stats'):
        assert hasattr(pkg.Engine, name), name
    src = open(os.path.join(ROOT, 'include', 'bpe.h')).read()
    body = re.search(r'typedef struct \{([^}]*)\} bpe_ingest_stats;', src).group(1)
    fields = re.findall(r'^\s*(int64_t|double)\s+(\w+);', body, re.M)
    assert [f[1] for f in fields] == [f[0] for f in pkg.IngestStats._fields_]
    assert ctypes.sizeof(pkg.IngestStats) == 8 * len(fields) == 48


# ---- GPU ------------------------------------------------------------------------------------------

def check_batch(e, units, off, table=None, nt0=None, tensors=False):
    """One flat call against restate_np: numbering, counts and the samples it appended."""
    nt0 = e.num_tokens() if nt0 is None else nt0
    ns0, ntok0 = e.corpus_size()
    new, hist, ids, id_off, table, nt = restate_np(units, off, table, nt0)
    if tensors:
        import torch
        got_new, got_hist = e.add_text_tensors(torch.from_numpy(units.view(np.int16)).cuda(),
                                               torch.from_numpy(np.asarray(off, np.int64)).cuda())
    else:
        got_new, got_hist = e.add_text_flat(units, off)
    assert got_new.tolist() == new
    assert e.num_tokens() == nt
    assert np.array_equal(got_hist, hist)
    assert e.corpus_size() == (ns0 + len(off) - 1, ntok0 + len(ids))
    got_ids, got_off = e.read_corpus()
    assert np.array_equal(got_ids[ntok0:], ids)
    assert np.array_equal(got_off[ns0:] - got_off[ns0], id_off)
    return table


@pytest.mark.gpu
@pytest.mark.parametrize('part', range(3))
def test_all_small_cases(part):
    """One add_text call per case on a fresh Engine (every third case per part): numbering, counts,
    corpus; for the 221 cases beyond latin1 (all of them hold a supplementary char or a lone
    surrogate: counted in the CPU test) the training that follows, which pins len16 = 2 through
    max_length."""
    bad = []
    n_beyond = 0
    for case in load_small()[part::3]:
        tt, n_chars = case['token_table'], len(case['token_table']) - len(case['merges'])
        e = pkg.Engine(0)
        new, hist = e.add_text(case['samples'])
        c = Corpus()
        for s in case['samples']:
            c.add(s)
        want_ids, want_off = c.flat()
        ids, off = e.read_corpus()
        ok = ([chr(cp) for cp in new.tolist()] == [t[0] for t in tt[:n_chars]] and
              hist.tolist() == [t[2] for t in tt[:n_chars]] and
              np.array_equal(ids, want_ids) and np.array_equal(off, want_off))
        if ok and beyond_latin1(case):
            n_beyond += 1
            o = case['opts']
            merges = e.merge_until(o.get('max_length') or 0, o.get('min_weight') or 0, o.get('max_iterations') or 0)
            ok = [list(m) for m in merges] == case['merges'] and e.samples() == case['final_ids']
        e.close()
        if not ok:
            bad.append(case['name'])
            if len(bad) > 5:
                break
    assert not bad, bad
    assert n_beyond == sum(beyond_latin1(c) for c in load_small()[part::3]) > 60


@pytest.mark.gpu
def test_edges_of_the_tiling():
    G, H, L = '\U0001F600', '\ud83d', '\ude00'
    batches = {
        'pair across a tile boundary': ['a' * (TILE - 1) + G + 'b' * 5],
        'text boundary between a high and a low surrogate, at a tile boundary': ['a' * (TILE - 1) + H, L + 'b', G],
        'text boundary between a high and a low surrogate, inside a lane': ['ab' + H, L + 'c' + G],
        'empty texts first, last, consecutive': ['', '', 'xy', '', '', '', G + 'z', ''],
        'empty texts at a tile\'s slot 0': ['q' * TILE, '', '', 'r' * 10, ''],
        'only empty texts': ['', '', ''],
        'a one-unit batch': ['k'],
        'a lone low first, a lone high last': [L + 'a' + H],
    }
    for what, texts in batches.items():
        e = pkg.Engine(0)
        new, hist, samples, _, nt = restate(texts)
        got_new, got_hist = e.add_text(texts)
        assert got_new.tolist() == new, what
        assert got_hist.tolist() == hist_list(hist, nt), what
        assert e.samples() == samples, what
        e.close()
    # a text boundary inside a pair makes two chars, distinct from the pair
    new, _, samples, _, _ = restate(['ab' + H, L + 'c' + G])
    assert new == [ord('a'), ord('b'), 0xD83D, 0xDE00, ord('c'), 0x1F600] and samples[1] == [3, 4, 5]
    # n_texts == 0
    e = pkg.Engine(0)
    new, hist = e.add_text([])
    assert new.size == 0 and hist.size == 0 and e.corpus_size() == (0, 0)
    # off[0] != 0: the units before it are never read (they would be new chars)
    units, off = pack(['hello', '', 'w' + G + 'rld'])
    junk = np.full(5, 0x4E2D, np.uint16)
    table = check_batch(e, np.concatenate([junk, units]), off + 5)
    assert 0x4E2D not in table
    # a unit pointer 2 B off 16-B alignment over three tiles (the device form: device_form_check)
    view, off = misaligned_batch()
    check_batch(e, view, off, table)
    e.close()


@pytest.mark.gpu
def test_more_tiles_than_a_scan_round():
    """Just over BPE_TEXT_SCAN_ROUND tiles: the scan carries across its rounds; pairs and text
    boundaries sit on both sides of the round's edge."""
    n = pkg.TEXT_SCAN_ROUND * TILE + TILE + 5
    rng = np.random.default_rng(11)
    units = rng.integers(0x4E00, 0x4E40, n, dtype=np.uint16)
    edge = pkg.TEXT_SCAN_ROUND * TILE
    for p in (edge - 1, edge + TILE - 1, 12345):
        units[p], units[p + 1] = 0xD840, 0xDC00 + (p & 0xFF)
    off = np.asarray([0, 1000, 1000, edge - 3, edge, edge + TILE, n, n], np.int64)
    e = pkg.Engine(0)
    check_batch(e, units, off)
    e.close()


@pytest.mark.gpu
def test_first_appearance():
    e = pkg.Engine(0)
    # the same new chars in many tiles: the least position wins; two new chars first seen in one
    # lane's run of 8 units; a new char at a tile's last unit against one at the next tile's first
    rng = np.random.default_rng(5)
    units = rng.integers(0x100, 0x100 + 50, 20 * TILE, dtype=np.uint16)
    units[:8] = [0x3000, 0x3001, 0x3000, 0x3002, 0x3003, 0x3001, 0x3004, 0x3005]
    units[TILE - 1], units[TILE] = 0x5000, 0x5001
    units[5 * TILE + 7], units[3 * TILE + 9], units[17 * TILE] = 0x5001, 0x5000, 0x5002
    off = np.asarray([0, 3, TILE + 1, 20 * TILE], np.int64)
    table = check_batch(e, units, off)
    # a batch with no new char
    ns = e.ingest_stats()['new_chars']
    check_batch(e, units, off, table)
    assert e.ingest_stats()['new_chars'] == ns
    # 3000 distinct supplementary chars: collisions in the insert, growth of the table's pair hash
    cps = 0x10000 + rng.choice(0x100000, 3000, replace=False)
    draw = rng.choice(cps, 20000)
    pairs = np.empty(2 * len(draw), np.uint16)
    pairs[0::2] = 0xD800 + ((draw - 0x10000) >> 10)
    pairs[1::2] = 0xDC00 + ((draw - 0x10000) & 0x3FF)
    table = check_batch(e, pairs, np.asarray([0, 2 * 7000, 2 * 7000, 2 * len(draw)], np.int64), table)
    # ... known now, mixed with BMP chars old and new
    mixed = np.concatenate([pairs[:4000], units[:100], np.asarray([0x6000, 0xD800, 0x6001], np.uint16), pairs[4000:8000]])
    check_batch(e, mixed, np.asarray([0, 5, len(mixed)], np.int64), table)
    e.close()


@pytest.mark.gpu
def test_one_batch_equals_one_call_per_text():
    rng = random.Random(21)
    alphabet = [chr(c) for c in range(0x61, 0x7B)] + ['中', 'Ж', '\U0001F600', '\U00020000', '\ud800', '\udc01']
    texts = [''.join(rng.choice(alphabet) for _ in range(rng.choice([0, 1, 3, 40, 300]))) for _ in range(60)]
    new, hist, samples, _, nt = restate(texts)
    a, b = pkg.Engine(0), pkg.Engine(0)
    new_a, hist_a = a.add_text(texts)
    new_b, hist_b = [], np.zeros(nt, np.int64)
    for t in texts:
        n1, h1 = b.add_text([t])
        new_b += n1.tolist()
        hist_b[:len(h1)] += h1
    assert new_a.tolist() == new_b == new
    assert hist_a.tolist() == hist_b.tolist() == hist_list(hist, nt)
    assert a.samples() == b.samples() == samples
    st = a.ingest_stats()
    assert (st['calls'], st['texts'], st['new_chars']) == (1, len(texts), nt)
    assert st['units'] == sum(len(units_of(t)) for t in texts) and st['chars'] == sum(map(len, samples))
    assert st['kernel_ms'] > 0
    a.close()
    b.close()


@pytest.mark.gpu
def test_a_batch_after_merges_numbers_past_them_and_training_goes_on():
    rng = random.Random(22)
    first = [''.join(rng.choice('abcd中\U0001F600') for _ in range(200)) for _ in range(8)]
    second = [''.join(rng.choice('abxyЖ\U00020000') for _ in range(200)) for _ in range(8)]
    e = pkg.Engine(0)
    e.add_text(first)
    c = Corpus()
    for t in first:
        c.add(t)
    st = OracleState.from_corpus(c)
    assert e.merge_until(3, 2, 12) == st.merge_until(3, 2, 12)
    nt0 = st.n_tokens
    assert e.num_tokens() == nt0 and nt0 > len(c.chars)
    table = {ord(ch): i for ch, i in c.char_to_index.items()}
    new, hist, samples, table, nt = restate(second, table, nt0)
    got_new, got_hist = e.add_text(second)
    assert got_new.tolist() == new and new and e.num_tokens() == nt
    assert got_hist.tolist() == hist_list(hist, nt)
    len16 = st.len16[:nt0].tolist() + [2 if cp > 0xFFFF else 1 for cp in new]
    ids = np.concatenate([st.ids] + [np.asarray(s, np.int32) for s in samples])
    off = np.concatenate([st.off, st.off[-1] + np.cumsum([len(s) for s in samples])])
    st2 = OracleState(ids, off, len16, nt)
    assert e.samples() == st2.samples()
    assert e.merge_until(3, 2, 12) == st2.merge_until(3, 2, 12)
    assert e.samples() == st2.samples()
    e.close()


@pytest.mark.gpu
def test_counts():
    e = pkg.Engine(0)
    # 2^20 units of one char
    check_batch(e, np.full(1 << 20, 0x4E2D, np.uint16), np.asarray([0, 1 << 19, 1 << 20], np.int64))
    e.close()
    # a uniform draw over 40 000 distinct BMP chars: most ids are outside any LDS-resident range
    e = pkg.Engine(0)
    rng = np.random.default_rng(9)
    units = np.concatenate([0x100 + rng.permutation(40000), rng.integers(0x100, 0x100 + 40000, 360000)]).astype(np.uint16)
    table = check_batch(e, units, np.asarray([0, 100000, 400000], np.int64))
    assert e.num_tokens() == 40000
    # a count past 2^16 for a char with a high id
    cp = next(c for c, i in table.items() if i == 39999)
    new, hist = e.add_text_flat(np.full(70001, cp, np.uint16), np.asarray([0, 70001], np.int64))
    assert new.size == 0 and hist[39999] == 70001 and hist.sum() == 70001
    e.close()


def raw_add(e, units, off, new_cap):
    new = np.zeros(max(new_cap, 1), np.uint32)
    hist = np.zeros(pkg.MAX_VOCAB, np.int64)
    n_new = ctypes.c_int64(-7)
    off = np.asarray(off, np.int64)
    rc = pkg.lib().bpe_add_text_batch(e._ctx, units.ctypes.data, off.ctypes.data_as(i64p), len(off) - 1,
                                      new.ctypes.data, new_cap, ctypes.byref(n_new), hist.ctypes.data_as(i64p),
                                      pkg.MAX_VOCAB)
    return rc, n_new.value, new


@pytest.mark.gpu
def test_failures_change_nothing():
    e = pkg.Engine(0)
    a = pkg.MAX_VOCAB - 4
    e.set_chars({'a': a})
    assert e.num_tokens() == pkg.MAX_VOCAB - 3   # room for 3 tokens
    e.add_text(['aaaa', 'aa'])

    def state():
        return e.corpus_size(), e.num_tokens(), e.find_next_merge(0, 2), e.samples()
    before = state()
    assert before[2] == (a, a, 3)
    with pytest.raises(pkg.BpeError) as err:
        e.add_text(['abc', 'de'])   # 4 new chars
    assert err.value.code == pkg.ERR_VOCAB
    assert state() == before
    # new_cap one too small: *n_new written, nothing changed, the retry succeeds
    units, off = pack(['ab', 'cd'])
    rc, n_new, _ = raw_add(e, units, off, 2)
    assert (rc, n_new) == (pkg.ERR_ARG, 3)
    assert state() == before
    # bad offsets
    for bad in ([0, 3, 2], [-1, 2, 4], [2, 1, 4]):
        rc, _, _ = raw_add(e, units, bad, 8)
        assert rc == pkg.ERR_ARG, bad
    assert state() == before
    # the next valid call numbers from the same id
    rc, n_new, new = raw_add(e, units, off, 3)
    assert (rc, n_new) == (0, 3) and new[:3].tolist() == [ord('b'), ord('c'), ord('d')]
    assert e.num_tokens() == pkg.MAX_VOCAB
    assert e.samples() == before[3] + [[a, a + 1], [a + 2, a + 3]]
    e.close()


@pytest.mark.gpu
@pytest.mark.parametrize('fresh', [True, False])
def test_multi_device_context(fresh):
    """Three shards on device 0 (reduce='host'): numbering, counts, read-back corpus and 50 merges
    equal one context's, on a fresh corpus (cut into runs) and after other samples (last shard)."""
    rng = random.Random(31)
    alphabet = [chr(c) for c in range(0x61, 0x6B)] + ['中', 'Ж', '\U0001F600', '\U00020000', '\ud800']
    texts = [''.join(rng.choice(alphabet) for _ in range(rng.choice([0, 5, 400, 3000]))) for _ in range(40)]
    one, multi = pkg.Engine(0), pkg.Engine(devices=[0, 0, 0], reduce='host')
    assert multi.shard_count() == 3
    if not fresh:
        for e in (one, multi):
            e.add_sample([0, 1, 1, 0])
            e.add_sample([1, 0])
    res = [e.add_text(texts) for e in (one, multi)]
    assert res[0][0].tolist() == res[1][0].tolist() and len(res[0][0]) == len(alphabet)
    assert res[0][1].tolist() == res[1][1].tolist()
    new, hist, samples, _, nt = restate(texts, None, 0 if fresh else 2)
    assert res[1][0].tolist() == new and res[1][1].tolist() == hist_list(hist, nt)
    assert one.num_tokens() == multi.num_tokens() == nt
    ids1, off1 = one.read_corpus()
    ids3, off3 = multi.read_corpus()
    assert np.array_equal(ids1, ids3) and np.array_equal(off1, off3)
    assert one.merge_until(4, 2, 50) == multi.merge_until(4, 2, 50)
    assert one.samples() == multi.samples()
    # a second batch goes to the last shard; known chars only
    res = [e.add_text(texts[:5]) for e in (one, multi)]
    assert res[0][0].size == res[1][0].size == 0 and res[0][1].tolist() == res[1][1].tolist()
    assert one.samples() == multi.samples()
    one.close()
    multi.close()


def misaligned_batch():
    """Three tiles of units whose pointer is 2 B off 16-B alignment, a pair across the first tile
    boundary of the 16-B cut, empty and boundary-crossing texts."""
    rng = np.random.default_rng(3)
    buf = np.zeros(3 * TILE + 16, np.uint16)
    k = ((2 - buf.ctypes.data) % 16) // 2
    view = buf[k:k + 3 * TILE]
    view[:] = rng.integers(0x61, 0x7B, 3 * TILE, dtype=np.uint16)
    view[TILE - 2], view[TILE - 1] = 0xD83D, 0xDE00   # (slots TILE - 1 and TILE of the tiles cut at 16 B)
    assert view.ctypes.data % 16 == 2
    return view, np.asarray([0, 7, 7, TILE + 3, len(view)], np.int64)


def device_form_check():
    """add_text_tensors equals the host form (a device pointer 2 B off 16-B alignment included), and
    an Encoder with the resulting char table and no merges encodes the texts to the corpus's samples."""
    import torch
    assert torch.cuda.is_available(), 'torch sees no device'
    rng = random.Random(41)
    alphabet = [chr(c) for c in range(0x61, 0x7B)] + ['中', '\U0001F600', '\U00020000', '\udc00']
    texts = [''.join(rng.choice(alphabet) for _ in range(rng.choice([0, 2, 100, 2500]))) for _ in range(30)]
    units, off = pack(texts)
    host, dev = pkg.Engine(0), pkg.Engine(0)
    new_h, hist_h = host.add_text_flat(units, off)
    table = check_batch(dev, units, off, tensors=True)
    assert new_h.tolist() == [cp for cp, _ in sorted(table.items(), key=lambda kv: kv[1])]
    assert host.samples() == dev.samples()
    # 2 B off 16-B alignment on the device: slot 0 of the first tile holds no unit of the batch
    view, voff = misaligned_batch()
    d = torch.zeros(len(view) + 1, dtype=torch.int16, device='cuda')[1:]
    d.copy_(torch.from_numpy(view.view(np.int16).copy()))
    assert d.data_ptr() % 16 == 2
    ns0, ntok0 = dev.corpus_size()
    new, hist, ids, id_off, table2, nt = restate_np(view, voff, table, dev.num_tokens())
    got_new, got_hist = dev.add_text_tensors(d, torch.from_numpy(voff).cuda())
    assert got_new.tolist() == new and np.array_equal(got_hist, hist)
    got_ids, got_off = dev.read_corpus()
    assert np.array_equal(got_ids[ntok0:], ids) and np.array_equal(got_off[ns0:] - got_off[ns0], id_off)
    # an empty device batch
    new, hist = dev.add_text_tensors(torch.zeros(0, dtype=torch.int16, device='cuda'),
                                     torch.zeros(1, dtype=torch.int64, device='cuda'))
    assert new.size == 0 and hist.sum() == 0
    enc = pkg.Encoder(0)
    enc.set_chars(table)
    got = enc.encode_text(texts, 'ids')
    assert [g.tolist() for g in got] == host.samples()
    for x in (host, dev, enc):
        x.close()
    return True


@pytest.mark.gpu
def test_device_form_and_round_trip_through_an_encoder():
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
