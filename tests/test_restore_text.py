"""Corpus from encoded samples and the restore on the device (bpe_add_sample_batch,
bpe_restore_text_batch, bpe_token_counts, include/bpe.h; csrc/bpe_append.hip.h): bpe_add_sample for a
batch, and restoreToCorpus (core.ts:213-216) for a batch of UTF-16 texts.

Expected values never come from the code under test:
  - slots():  a numpy restatement of the appended region (g[k] = off[k] - off[0] + k, sample k's
              separator in slot g[k+1] - 1), pinned against oracle.Corpus.flat() on every golden case;
  - the golden cases' final_ids: the reference's trained corpus is encodeToCode of each raw sample, so
    restoring a case's samples with its chars and merges gives final_ids exactly;
  - oracle.encode, oracle.Corpus / OracleState, and contexts built by bpe_add_sample per sample.
"""
import ctypes
import functools
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

T = pkg.APPEND_TILE
SEP = -1
i64p = ctypes.POINTER(ctypes.c_int64)


def units_of(text):
    return np.frombuffer(text.encode('utf-16-le', 'surrogatepass'), dtype='<u2').astype(np.uint16)


def pack(texts):
    parts = [units_of(t) for t in texts]
    off = np.zeros(len(parts) + 1, np.int64)
    np.cumsum([len(p) for p in parts], out=off[1:])
    units = np.concatenate(parts) if parts and off[-1] else np.zeros(0, np.uint16)
    return units, off


def slots(ids, off):
    """The appended region of n samples: total + n slots, every sample's ids then a separator."""
    off = np.asarray(off, np.int64)
    n = len(off) - 1
    base, total = (int(off[0]), int(off[-1] - off[0])) if n else (0, 0)
    g = off - base + np.arange(n + 1)
    out = np.full(total + n, SEP, np.int32)
    k_of = np.repeat(np.arange(n), np.diff(off))
    out[np.arange(total) + k_of] = np.asarray(ids, np.int32)[base:base + total]
    assert n == 0 or (out[g[1:] - 1] == SEP).all()
    return out, g


def samples_of_slots(region):
    out, cur = [], []
    for x in region.tolist():
        if x == SEP:
            out.append(cur)
            cur = []
        else:
            cur.append(x)
    assert not cur
    return out


def case_vocab(case):
    """(chars in first-appearance order, (a, b, c) merges, len16 per token id) of a golden case."""
    tt = case['token_table']
    n_chars = len(tt) - len(case['merges'])
    chars = [t[0] for t in tt[:n_chars]]
    merges = [(a, b, n_chars + i) for i, (a, b, _w) in enumerate(case['merges'])]
    len16 = [len(t[0].encode('utf-16-le', 'surrogatepass')) // 2 for t in tt]
    return chars, merges, len16


# ---- CPU ------------------------------------------------------------------------------------------

def test_new_names_are_exported_and_append_stats_match_the_header():
    for name in ('bpe_add_sample_batch', 'bpe_add_sample_batch_device', 'bpe_restore_text_batch',
                 'bpe_restore_text_batch_device', 'bpe_token_counts', 'bpe_get_append_stats',
                 'bpe_reset_append_stats'):
        assert name in pkg.C_API
        assert hasattr(pkg.lib(), name), name
    for name in ('add_samples_flat', 'add_samples', 'add_samples_tensors', 'restore_text', 'restore_text_flat',
                 'restore_text_tensors', 'token_counts', 'append_stats', 'reset_append_stats'):
        assert hasattr(pkg.Engine, name), name
    src = open(os.path.join(ROOT, 'include', 'bpe.h')).read()
    body = re.search(r'typedef struct \{([^}]*)\} bpe_append_stats;', src).group(1)
    fields = re.findall(r'^\s*(int64_t|double)\s+(\w+);', body, re.M)
    assert [f[1] for f in fields] == [f[0] for f in pkg.AppendStats._fields_] == ['calls', 'samples', 'tokens', 'kernel_ms']
    assert [f[0] for f in fields] == ['int64_t', 'int64_t', 'int64_t', 'double']
    assert [f[1] for f in pkg.AppendStats._fields_] == [ctypes.c_int64] * 3 + [ctypes.c_double]
    assert ctypes.sizeof(pkg.AppendStats) == 8 * len(fields) == 32
    assert pkg.APPEND_TILE == 2048 == int(re.search(r'#define BPE_APPEND_TILE (\d+)', src).group(1))


def test_slot_layout_restatement_on_the_golden_cases():
    cases = load_small()
    assert len(cases) == 1509
    n_empty = 0
    for case in cases:
        c = Corpus()
        for s in case['final_ids']:
            c.add_ids(s)
            n_empty += not s
        assert sum(not s for s in case['samples']) == sum(not s for s in case['final_ids'])
        ids, off = c.flat()
        for lead in (0, 3):
            region, g = slots(np.concatenate([np.full(lead, 9999, np.int32), ids]), off + lead)
            assert len(region) == len(ids) + len(case['final_ids'])
            assert samples_of_slots(region) == case['final_ids'], case['name']
            assert np.array_equal(np.flatnonzero(region == SEP), g[1:] - 1)
    assert n_empty == 571


# ---- GPU ------------------------------------------------------------------------------------------

def state_of(e):
    ids, off = e.read_corpus()
    return e.corpus_size(), e.num_tokens(), ids.copy(), off.copy(), e.token_counts()


def same_state(a, b):
    return a[0] == b[0] and a[1] == b[1] and all(np.array_equal(x, y) for x, y in zip(a[2:], b[2:]))


def check_append(e, ids, off, what=''):
    """One add_samples_flat call against the restatement: the corpus, its offsets and the counts."""
    (ns0, ntok0), nt0, ids0, off0, _ = state_of(e)
    off = np.asarray(off, np.int64)
    region, g = slots(ids, off)
    e.add_samples_flat(ids, off)
    want_ids = np.concatenate([ids0, region[region != SEP]])
    want_off = np.concatenate([off0, off0[-1] + (g[1:] - np.arange(1, len(g)))])
    got_ids, got_off = e.read_corpus()
    assert np.array_equal(got_ids, want_ids), what
    assert np.array_equal(got_off, want_off), what
    nt = max(nt0, int(want_ids.max()) + 1 if want_ids.size else 0)
    assert e.num_tokens() == nt, what
    assert e.corpus_size() == (ns0 + len(off) - 1, len(want_ids)), what
    assert np.array_equal(e.token_counts(), np.bincount(want_ids, minlength=nt)), what


@pytest.mark.gpu
@pytest.mark.parametrize('part', range(3))
def test_all_small_cases(part):
    """One restore call per case into a fresh context (every third case per part): the corpus is the
    case's final_ids, the counts its bincount, the next merge the oracle's on that corpus."""
    bad = []
    enc = pkg.Encoder(0)
    for case in load_small()[part::3]:
        chars, merges, len16 = case_vocab(case)
        enc.clear()
        enc.set_chars({ch: i for i, ch in enumerate(chars)})
        if merges:
            enc.add_merges(merges)
        e = pkg.Engine(0)
        for i, l in enumerate(len16):
            e.set_token_len16(i, l)
        e.restore_text(enc, case['samples'])
        c = Corpus()
        for s in case['final_ids']:
            c.add_ids(s)
        want_ids, want_off = c.flat()
        ids, off = e.read_corpus()
        ok = np.array_equal(ids, want_ids) and np.array_equal(off, want_off)
        ok = ok and e.num_tokens() == len(len16)
        ok = ok and np.array_equal(e.token_counts(), np.bincount(want_ids, minlength=len(len16)))
        if ok:
            st = OracleState(want_ids, want_off, len16, len(len16))
            ok = e.find_next_merge(0, 0) == st.find_next_merge(None, None)
        e.close()
        if not ok:
            bad.append(case['name'])
            if len(bad) > 5:
                break
    enc.close()
    assert not bad, bad


def edge_batches():
    """Sample lengths of every edge case (a sample of m tokens ends, with its separator, at slot
    m of the region when it is the first)."""
    out = {}
    for p in (T - 2, T - 1, T, T + 1, 2 * T - 1, 2 * T, 2 * T + 1):
        out['a sample end at slot %d' % p] = [p, 5]
    out['a tile in which nothing ends'] = [3 * T + 5]
    out['T + 3 empty samples across a tile edge'] = [T - 2] + [0] * (T + 3) + [7]
    out['a tile of separators only, whatever the residue'] = [T - 6] + [0] * (T + 8) + [7]
    out['an empty first and an empty last sample'] = [0, 5, 0]
    out['n = 0'] = []
    out['one empty sample'] = [0]
    return out


@pytest.mark.gpu
@pytest.mark.parametrize('residue', range(4))
def test_tiling_edges(residue):
    """Every edge case appended where live_slots mod 4 is `residue` (an unaligned destination), with
    ids below 300 and up to 20 000 (both histogram paths), from source offset 0 and from an odd one."""
    rng = np.random.default_rng(100 + residue)
    for what, lens in edge_batches().items():
        for top in (300, 20000):
            for lead in (0, 5):
                e = pkg.Engine(0)
                e.add_sample([1] * (residue + 3))   # residue + 4 slots
                total = int(sum(lens))
                ids = np.concatenate([np.full(lead, pkg.MAX_VOCAB + 7, np.int32),   # (never read)
                                      rng.integers(0, top, total, dtype=np.int32)])
                off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64) + lead
                check_append(e, ids, off, (what, top, lead))
                e.close()


@pytest.mark.gpu
def test_one_batch_equals_one_call_per_sample_equals_a_loop_of_add_sample():
    rng = np.random.default_rng(23)
    samples = [rng.integers(0, 500, rng.choice([0, 1, 3, 40, 300, 5000])).astype(np.int32) for _ in range(60)]
    a, b, c = pkg.Engine(0), pkg.Engine(0), pkg.Engine(0)
    a.add_samples(samples)
    for s in samples:
        b.add_samples([s])
        c.add_sample(s)
    want = state_of(c)
    assert same_state(state_of(a), want) and same_state(state_of(b), want)
    lens = [len(s) for s in samples]
    assert a.sample_lengths().tolist() == b.sample_lengths().tolist() == c.sample_lengths().tolist() == lens
    flat = Corpus()
    for s in samples:
        flat.add_ids(s)
    ids, off = flat.flat()
    nt = a.num_tokens()
    assert nt == int(ids.max()) + 1
    st = OracleState(ids, off, [1] * nt, nt)
    m = st.merge_until(None, 2, 50)
    assert len(m) == 50
    assert a.merge_until(0, 2, 50) == b.merge_until(0, 2, 50) == c.merge_until(0, 2, 50) == m
    assert a.samples() == b.samples() == c.samples() == st.samples()
    for e in (a, b, c):
        e.close()


@functools.lru_cache(maxsize=None)
def zipf_run():
    """A small zipf-words corpus (1 MiB, samples of 4 KiB) and the oracle's 300 merges on it:
    (bytes, char ids, merges, the oracle's samples after 200 merges, the oracle's state after 300)."""
    data = pkg.synth_zipf(1 << 20, seed=5, sample_bytes=4096)
    _uniq, first = np.unique(data, return_index=True)
    cmap = np.full(256, -1, np.int32)
    for i, p in enumerate(np.sort(first)):
        cmap[data[p]] = i
    nt = int((cmap >= 0).sum())
    ids = cmap[data].astype(np.int32)
    off = np.arange(0, len(data) + 1, 4096, dtype=np.int64)
    st = OracleState(ids, off, [1] * nt, nt)
    merges = st.merge_until(None, 2, 200)
    after_200 = (st.ids[:st.off[-1]].copy(), st.off.copy())
    merges += st.merge_until(None, 2, 100)
    assert len(merges) == 300
    return data, cmap, nt, merges, after_200, st


@pytest.mark.gpu
@pytest.mark.parametrize('mode', ['stream', 'incremental'])
def test_resume(mode):
    """Engine A trains 200 merges; engine B and an encoder are built from A's chars and merges, B
    registers the tokens and restores the raw texts: B's corpus is A's, and 100 further merges are
    the same in A, B and the oracle."""
    from test_maintained_state import check_maintained
    data, cmap, nt, merges, after_200, st = zipf_run()
    a = pkg.Engine(0)
    a.set_mode(mode)
    got_cmap, got_nt, _hist = a.add_latin1(data, sample_bytes=4096)
    assert got_nt == nt and np.array_equal(got_cmap, cmap)
    assert a.merge_until(0, 2, 200) == merges[:200]
    b = pkg.Engine(0)
    b.set_mode(mode)
    len16 = [1] * nt
    for x, y, _w in merges[:200]:
        len16.append(len16[x] + len16[y])
    for i, l in enumerate(len16):
        b.set_token_len16(i, l)
    enc = pkg.Encoder(0, [(x, y, nt + i) for i, (x, y, _w) in enumerate(merges[:200])])
    enc.set_chars({int(ch): int(cmap[ch]) for ch in range(256) if cmap[ch] >= 0})
    b.restore_text_flat(enc, data.astype(np.uint16), np.arange(0, len(data) + 1, 4096, dtype=np.int64))
    ids_a, off_a = a.read_corpus()
    ids_b, off_b = b.read_corpus()
    assert np.array_equal(ids_b, after_200[0]) and np.array_equal(off_b, after_200[1])
    assert np.array_equal(ids_a, ids_b) and np.array_equal(off_a, off_b)
    assert np.array_equal(b.token_counts(), np.bincount(ids_b, minlength=nt + 200))
    assert a.merge_until(0, 2, 100) == merges[200:]
    assert b.merge_until(0, 2, 100) == merges[200:]
    ids_b, off_b = b.read_corpus()
    assert np.array_equal(ids_b, st.ids[:st.off[-1]]) and np.array_equal(off_b, st.off)
    assert np.array_equal(b.token_counts(), np.bincount(ids_b, minlength=nt + 300))
    if b.is_maintained():
        check_maintained(b, st)
    for x in (a, b, enc):
        x.close()


@pytest.mark.gpu
def test_restore_after_merges_into_a_live_corpus():
    rng = random.Random(24)
    first = [''.join(rng.choice('abcd中\U0001F600') for _ in range(300)) for _ in range(8)]
    second = [''.join(rng.choice('abcd中\U0001F600') for _ in range(rng.choice([0, 7, 300, 2500]))) for _ in range(9)]
    e = pkg.Engine(0)
    e.add_text(first)
    c = Corpus()
    for t in first:
        c.add(t)
    st = OracleState.from_corpus(c)
    m = st.merge_until(3, 2, 12)
    assert e.merge_until(3, 2, 12) == m and len(m) == 12
    n_chars = len(c.chars)
    abc = [(a, b, n_chars + i) for i, (a, b, _w) in enumerate(m)]
    enc = pkg.Encoder(0, abc)
    enc.set_chars(dict(c.char_to_index))
    e.restore_text(enc, second)
    want = oracle.encode([[c.char_to_index[ch] for ch in t] for t in second], abc)
    ids = np.concatenate([st.ids[:st.off[-1]]] + [np.asarray(w, np.int32) for w in want])
    off = np.concatenate([st.off, st.off[-1] + np.cumsum([len(w) for w in want])])
    st2 = OracleState(ids, off, st.len16[:st.n_tokens].tolist(), st.n_tokens)
    assert e.num_tokens() == st.n_tokens
    assert e.samples() == st2.samples()
    assert np.array_equal(e.token_counts(), np.bincount(ids, minlength=st.n_tokens))
    m2 = st2.merge_until(3, 2, 12)
    assert e.merge_until(3, 2, 12) == m2 and m2
    assert e.samples() == st2.samples()
    e.close()
    enc.close()


@pytest.mark.gpu
def test_long_texts_replayed_and_split():
    """A golden case's merge list, and a char of no merge planted every few thousand chars (a
    boundary beside it is one no merge can cross): the default mode replays the long texts on the
    host, the split mode keeps them on the device; both give oracle.encode's ids in the corpus."""
    from test_encoder_split import split_ok
    case = next(c for c in load_small()
                if len(c['merges']) >= 20 and split_ok(case_vocab(c)[1]) and 'Ω' not in case_vocab(c)[0]
                and 4 <= len(case_vocab(c)[0]) and all(len(ch.encode('utf-16-le', 'surrogatepass')) == 2
                                                       for ch in case_vocab(c)[0]))
    chars, merges, len16 = case_vocab(case)
    extra = len(len16)   # the planted char: an id past the merged tokens
    rng = np.random.default_rng(25)
    texts_ids = []
    for n in (pkg.ENCODE_LDS_TOKENS + 1 + 300, 40000, 50):
        t = rng.integers(0, len(chars), n).astype(np.int32)
        t[np.arange(1000, n, 3000)] = extra
        texts_ids.append(t)
    alphabet = chars + ['Ω']
    texts = [''.join(alphabet[i if i != extra else len(chars)] for i in t) for t in texts_ids]
    want = [w.tolist() for w in oracle.encode(texts_ids, merges)]
    table = {ch: i for i, ch in enumerate(chars)}
    table['Ω'] = extra
    for mode in ('replay', 'split'):
        enc = pkg.Encoder(0, merges, long_texts=mode)
        enc.set_chars(table)
        e = pkg.Engine(0)
        e.restore_text(enc, texts)
        if mode == 'replay':
            assert enc.stats()['texts_replay'] > 0
        else:
            assert enc.split_stats()['texts_split'] == 2 and enc.split_stats()['texts_fallback'] == 0
            assert enc.stats()['texts_replay'] == 0   # (no host assembly)
        assert e.samples() == want, mode
        assert e.num_tokens() == extra + 1
        assert np.array_equal(e.token_counts(), np.bincount(np.concatenate(want), minlength=extra + 1))
        e.close()
        enc.close()


def raw_restore(e, enc_ptr, units, off):
    off = np.asarray(off, np.int64)
    rc = pkg.lib().bpe_restore_text_batch(e._ctx, enc_ptr, units.ctypes.data, off.ctypes.data_as(i64p), len(off) - 1)
    return rc, pkg.last_error()


def raw_add(e, ids, off):
    off = np.asarray(off, np.int64)
    ids = np.ascontiguousarray(ids, np.int32)
    rc = pkg.lib().bpe_add_sample_batch(e._ctx, ids.ctypes.data, off.ctypes.data_as(i64p), len(off) - 1)
    return rc, pkg.last_error()


@pytest.mark.gpu
def test_failures_change_nothing():
    """Every failing batch spans several tiles and starts mid-chunk, with the bad entry late: the
    kernel has overwritten the sealed tail of the last chunk before the call fails."""
    rng = np.random.default_rng(26)
    chars = 'abcdefgh'
    first = [''.join(chars[i] for i in rng.integers(0, 8, 700)) for _ in range(5)]
    e = pkg.Engine(0)
    e.add_text(first)
    c = Corpus()
    for t in first:
        c.add(t)
    st = OracleState.from_corpus(c)
    m = st.merge_until(None, 2, 6)
    assert e.merge_until(0, 2, 6) == m
    abc = [(a, b, 8 + i) for i, (a, b, _w) in enumerate(m)]
    enc = pkg.Encoder(0, abc)
    enc.set_chars(dict(c.char_to_index))
    before = state_of(e)
    assert before[0][0] == 5 and before[1] == 14

    good = [''.join(chars[i] for i in rng.integers(0, 8, 3000)) for _ in range(4)]
    # an unknown char, late in the batch
    texts = good + ['ab' + 'z' + 'cd']
    units, off = pack(texts)
    rc, msg = raw_restore(e, enc._enc, units, off)
    assert rc == pkg.ERR_VOCAB and msg == 'unknown token, char: U+007A (text 4, unit 2)', msg
    assert same_state(state_of(e), before)
    # an encoder without a char table
    bare = pkg.Encoder(0, abc)
    rc, _ = raw_restore(e, bare._enc, *pack(good))
    assert rc == pkg.ERR_STATE
    bare.close()
    # decreasing and negative offsets, both entry points
    units, off = pack(good)
    for bad in ([0, 30, 20, 40], [-1, 5, 9], [5, 4]):
        assert raw_restore(e, enc._enc, units, bad)[0] == pkg.ERR_ARG, bad
        assert raw_add(e, np.zeros(64, np.int32), bad)[0] == pkg.ERR_ARG, bad
    # a null encoder
    assert raw_restore(e, None, units, off)[0] == pkg.ERR_ARG
    assert same_state(state_of(e), before)
    # ids out of range, late in a batch of several tiles
    for bad_id in (pkg.MAX_VOCAB, -1):
        ids = rng.integers(0, 14, 5 * T).astype(np.int32)
        ids[-3] = bad_id
        rc, msg = raw_add(e, ids, [0, 10, 10, 3 * T, 5 * T])
        assert rc == pkg.ERR_ARG and msg == 'bpe native: token id out of range in sample', (bad_id, msg)
        assert same_state(state_of(e), before)
    # the corpus still trains as the oracle's, and takes the good batch afterwards
    m2 = st.merge_until(None, 2, 5)
    assert e.merge_until(0, 2, 5) == m2 and len(m2) == 5
    assert e.samples() == st.samples()
    e.close()
    enc.close()


@pytest.mark.gpu
@pytest.mark.parametrize('fresh', [True, False])
def test_multi_device_context(fresh):
    """Three shards on device 0 (reduce='host'): corpus, counts and 50 merges equal one context's,
    on a fresh corpus (cut into runs) and after other samples (last shard), for both entry points."""
    rng = np.random.default_rng(31)
    samples = [rng.integers(0, 40, rng.choice([0, 5, 400, 3000])).astype(np.int32) for _ in range(40)]
    chars = [chr(0x61 + i) for i in range(20)] + ['中', '\U0001F600']
    texts = [''.join(chars[i] for i in rng.integers(0, len(chars), rng.choice([0, 9, 900]))) for _ in range(12)]
    texts[0] = 'abcab' + texts[0]
    enc = pkg.Encoder(0, [(0, 1, 40), (40, 2, 41)])
    enc.set_chars({ch: i for i, ch in enumerate(chars)})
    one, multi = pkg.Engine(0), pkg.Engine(devices=[0, 0, 0], reduce='host')
    assert multi.shard_count() == 3
    for e in (one, multi):
        if not fresh:
            e.add_sample([0, 1, 1, 0])
            e.add_sample([1, 0])
        e.add_samples(samples)
        e.restore_text(enc, texts)
    assert same_state(state_of(one), state_of(multi))
    assert one.num_tokens() == 42
    st = multi.append_stats()
    assert (st['calls'], st['samples']) == (2, len(samples) + len(texts))
    assert one.merge_until(4, 2, 50) == multi.merge_until(4, 2, 50)
    assert same_state(state_of(one), state_of(multi))
    for x in (one, multi, enc):
        x.close()


@pytest.mark.gpu
def test_append_stats():
    e = pkg.Engine(0)
    assert e.append_stats() == dict(calls=0, samples=0, tokens=0, kernel_ms=0.0)
    e.add_samples([])
    st = e.append_stats()
    assert (st['calls'], st['samples'], st['tokens'], st['kernel_ms']) == (1, 0, 0, 0.0)
    e.add_samples([[1, 2, 3], [], [4]])
    enc = pkg.Encoder(0, [(0, 1, 2)])
    enc.set_chars({'a': 0, 'b': 1})
    e.restore_text(enc, ['abab', 'b'])
    st = e.append_stats()
    assert (st['calls'], st['samples'], st['tokens']) == (3, 5, 4 + 3) and st['kernel_ms'] > 0
    assert e.samples() == [[1, 2, 3], [], [4], [2, 2], [1]]
    with pytest.raises(pkg.BpeError):
        e.add_samples([[1, pkg.MAX_VOCAB]])
    st = e.append_stats()
    assert (st['calls'], st['samples'], st['tokens']) == (4, 5, 7)
    e.reset_append_stats()
    assert e.append_stats() == dict(calls=0, samples=0, tokens=0, kernel_ms=0.0)
    e.close()
    enc.close()


def device_form_check():
    """restore_text_tensors and add_samples_tensors on torch tensors, then read_corpus and
    Decoder.decode give the texts back (supplementary chars and lone surrogates included)."""
    import torch
    assert torch.cuda.is_available(), 'torch sees no device'
    rng = random.Random(41)
    alphabet = [chr(c) for c in range(0x61, 0x6B)] + ['中', '\U0001F600', '\U00020000', '\udc00']
    texts = [''.join(rng.choice(alphabet) for _ in range(rng.choice([0, 2, 100, 2500, 5000]))) for _ in range(30)]
    texts = [t + '\ud801' if k % 4 == 0 else t for k, t in enumerate(texts)]   # (a lone high: at a text's end)
    c = Corpus()
    for t in texts:
        c.add(t)
    st = OracleState.from_corpus(c)
    m = st.merge_until(None, 2, 40)
    n_chars = len(c.chars)
    abc = [(a, b, n_chars + i) for i, (a, b, _w) in enumerate(m)]
    enc = pkg.Encoder(0, abc)
    enc.set_chars(dict(c.char_to_index))
    units, off = pack(texts)
    e = pkg.Engine(0)
    e.add_sample([3, 3])   # (an unaligned destination)
    # a device pointer 2 B off 16-B alignment, and offsets that do not start at 0
    d = torch.zeros(len(units) + 8, dtype=torch.int16, device='cuda')[1:]
    d[7:7 + len(units)].copy_(torch.from_numpy(units.view(np.int16).copy()))
    assert d.data_ptr() % 16 == 2
    e.restore_text_tensors(enc, d, torch.from_numpy(off + 7).cuda())
    assert e.samples() == [[3, 3]] + st.samples()
    dec = pkg.Decoder(0)
    dec.add_tokens(c.chars)
    dec.add_merges(abc)
    assert dec.decode(e.samples()[1:], 'ids') == texts
    # the sample form on tensors: an odd source offset
    ids, ioff = e.read_corpus()
    f = pkg.Engine(0)
    dv = torch.from_numpy(np.concatenate([np.full(3, -5, np.int32), ids])).cuda()
    f.add_samples_tensors(dv, torch.from_numpy(ioff + 3).cuda())
    assert f.samples() == e.samples() and np.array_equal(f.token_counts(), e.token_counts())
    # empty device batches
    f.add_samples_tensors(torch.zeros(0, dtype=torch.int32, device='cuda'), torch.zeros(1, dtype=torch.int64, device='cuda'))
    f.restore_text_tensors(enc, torch.zeros(0, dtype=torch.int16, device='cuda'), torch.zeros(2, dtype=torch.int64, device='cuda'))
    assert f.samples() == e.samples() + [[]]
    for x in (e, f, enc, dec):
        x.close()
    return True


@pytest.mark.gpu
def test_device_form_and_round_trip_through_a_decoder():
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
