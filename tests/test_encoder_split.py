"""Long texts in segments (BPE_LONG_SPLIT, csrc/bpe_encode.hip: k_cuts and the planner): a text of
more than ENCODE_LDS_TOKENS tokens is cut at boundaries no merge can cross and its segments go
through the merge-rank kernels.  Checked against

  - the whole-text replay (oracle.encode) for the outputs, and
  - `plan_text`, the Python restatement of the plan (first / last base id of every id, the cut
    set, windows of ENCODE_SPLIT_WINDOW boundaries, the largest safe boundary of each), for
    `segments`, `texts_split` and `texts_fallback`.

The CPU tests at the bottom pin the rule itself: at toy caps, the replays of the segments of
`plan_text`, concatenated, equal the replay of the whole text.
"""
import ctypes
import functools

import numpy as np
import pytest

import oracle
from bpe_amd import pkg
from oracle import Corpus, OracleState

H = pkg.ENCODE_SPLIT_WINDOW
CAP = pkg.ENCODE_LDS_TOKENS


# ---- the Python restatement of the plan -----------------------------------------------------------

def ends_and_cut_set(merges):
    """first[id], last[id] (arrays over MAX_VOCAB: identity for an id no merge makes) and the cut
    set as sorted keys last(a) << 16 | first(b), in list order."""
    first = np.arange(pkg.MAX_VOCAB, dtype=np.int64)
    last = first.copy()
    keys = set()
    for a, b, c in merges:
        keys.add((int(last[a]) << 16) | int(first[b]))
        first[c], last[c] = first[a], last[b]
    return first, last, np.asarray(sorted(keys), np.int64)


def split_ok(merges):
    """The lists the split route takes: no c is an input of its own or an earlier merge (the
    greedy's condition), and no id is made twice."""
    inputs, made = set(), set()
    for a, b, c in merges:
        inputs |= {a, b}
        if c in inputs or c in made:
            return False
        made.add(c)
    return True


def plan_text(text, tables, h, cap):
    """The segment starts of one text (its cuts after a leading 0), or None when it falls back; a
    text of at most `cap` tokens is never cut."""
    n = len(text)
    if n <= cap:
        return [0]
    first, last, keys = tables
    t = np.asarray(text, np.int64)
    ok = (t >= 0) & (t < pkg.MAX_VOCAB)
    tc = np.where(ok, t, 0)
    safe = np.zeros(n, bool)                                  # safe[p]: boundary p, 1 <= p <= n - 1
    safe[1:] = ~np.isin((last[tc[:-1]] << 16) | first[tc[1:]], keys) & ok[:-1] & ok[1:]
    cuts = []
    for lo in range(1, n, h):                                 # window j: [j h + 1, min((j + 1) h, n - 1)]
        hi = min(lo + h - 1, n - 1)
        p = np.flatnonzero(safe[lo:hi + 1])
        if len(p):
            cuts.append(lo + int(p[-1]))
    edges = [0] + cuts + [n]
    if max(b - a for a, b in zip(edges, edges[1:])) > cap:
        return None
    return [0] + cuts


def plan_stats(texts, merges, h=H, cap=CAP):
    """(segments, texts_split, texts_fallback, windows) of a call, and every text's plan."""
    tables = ends_and_cut_set(merges)
    plans = [plan_text(t, tables, h, cap) for t in texts]
    if not split_ok(merges):
        return dict(segments=0, texts_split=0, texts_fallback=0, windows=0), plans
    long = [(t, p) for t, p in zip(texts, plans) if len(t) > cap]
    return dict(segments=sum(len(p) for _t, p in long if p is not None),
                texts_split=sum(p is not None for _t, p in long),
                texts_fallback=sum(p is None for _t, p in long),
                windows=sum((len(t) - 2) // h + 1 for t, _p in long)), plans


# ---- lists and texts ------------------------------------------------------------------------------

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


def random_texts(rng, alphabet, lengths):
    return [rng.integers(0, alphabet, size=l).astype(np.int32) for l in lengths]


def skewed_texts(rng, alphabet, lengths):
    """Texts with long runs and repeats (x == y pairs)."""
    out = []
    for l in lengths:
        t = np.empty(l, np.int32)
        i = 0
        while i < l:
            run = int(rng.integers(1, 40))
            t[i:i + run] = rng.integers(0, max(1, alphabet // 4))
            i += run
        out.append(t)
    return out


@functools.lru_cache(maxsize=None)
def fixture_a():
    """A list over the ids 0..7 whose cut set holds all 64 of their pairs, with the ids 8 and 9 in
    no merge: a boundary is safe iff it touches an 8 (or a 9)."""
    merges = trained_merges(np.random.default_rng(21), 8, 40, 300)
    sh = lambda x: x + 2 if x >= 8 else x
    merges = [(sh(a), sh(b), sh(c)) for a, b, c in merges]
    _f, _l, keys = ends_and_cut_set(merges)
    assert len(merges) == 461
    assert sorted(keys.tolist()) == sorted((x << 16) | y for x in range(8) for y in range(8))
    return merges


def planted(rng, n, at, fill=8):
    t = rng.integers(0, 8, size=n).astype(np.int32)
    t[list(at)] = fill
    return t


def planted_cases(rng, h=H, cap=CAP):
    """The six texts of fixture A, and their segment counts at the real cap (None: falls back).
    The third one's count follows the window: worked out on the CPU for each of the four windows
    the bench compared (2048 was the first default)."""
    third = {1024: 47, 2048: 23, 4096: 11, 8192: None}.get(h)
    return [
        (planted(rng, cap + 1, [1]), 2),
        (planted(rng, cap + 1, [cap]), 2),
        (planted(rng, 3 * cap + 5, [h, h + 1, 2 * h - 1, 5 * h] + list(range(7 * h, 3 * cap + 5, h - 3))), third),
        (planted(rng, 2 * cap, [cap - 1, cap + 5]), 3),
        (planted(rng, cap + 1, []), None),
        (planted(rng, 3 * cap, [100, 101 + cap]), None),
    ]


@functools.lru_cache(maxsize=None)
def planted_with_reference():
    """The planted texts with their whole-text replays, made once for the tests that share them."""
    cases = planted_cases(np.random.default_rng(5))
    texts = [t for t, _n in cases]
    return texts, [n for _t, n in cases], oracle.encode(texts, fixture_a())


def split_encoder(merges):
    enc = pkg.Encoder(0, merges, long_texts='split')
    enc.reset_stats()
    enc.reset_split_stats()
    return enc


def check_split(enc, texts, merges, want=None):
    """One call: outputs equal the whole-text replay, the split stats the Python plan's, and only
    the texts that fall back are replayed.  Returns the plan's counts."""
    enc.reset_stats()
    enc.reset_split_stats()
    got = enc.encode(texts)
    want = oracle.encode(texts, merges) if want is None else want
    for k, (g, w) in enumerate(zip(got, want)):
        assert g.tolist() == w.tolist(), 'text %d (len %d)' % (k, len(texts[k]))
    exp, _plans = plan_stats(texts, merges)
    st, ss = enc.stats(), enc.split_stats()
    print('split stats', ss, 'plan', exp)
    for key, v in exp.items():
        assert ss[key] == v, (key, ss, exp)
    n_long = sum(len(t) > CAP for t in texts)
    assert ss['calls'] == (1 if exp['windows'] else 0)
    if exp['windows']:
        assert st['texts_replay'] == exp['texts_fallback']
        assert st['texts_rank'] == len(texts) - exp['texts_fallback']
    else:                                                     # (no plan: the default route's counts)
        assert st['texts_replay'] >= n_long and st['texts_rank'] + st['texts_replay'] == len(texts)
    return exp


# ---- 1. planted boundaries ------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize('k', range(6))
def test_planted_boundaries_one_text(k):
    texts, n_seg, want = planted_with_reference()
    enc = split_encoder(fixture_a())
    try:
        exp = check_split(enc, [texts[k]], fixture_a(), [want[k]])
        if n_seg[k] is None:
            assert (exp['texts_split'], exp['texts_fallback'], exp['segments']) == (0, 1, 0)
        else:
            assert (exp['texts_split'], exp['texts_fallback'], exp['segments']) == (1, 0, n_seg[k])
    finally:
        enc.close()


@pytest.mark.gpu
def test_planted_boundaries_one_call_and_the_flat_form():
    """All six with short and empty texts between them, and the same ids through encode_flat with
    off[0] != 0."""
    texts, n_seg, want = planted_with_reference()
    rng = np.random.default_rng(6)
    short = random_texts(rng, 8, [0, 1, 700, 0, CAP, 64, 0])
    want_short = oracle.encode(short, fixture_a())
    mixed, want_mixed = [], []
    for k in range(6):
        mixed += [short[k], texts[k]]
        want_mixed += [want_short[k], want[k]]
    mixed.append(short[6])
    want_mixed.append(want_short[6])
    enc = split_encoder(fixture_a())
    try:
        exp = check_split(enc, mixed, fixture_a(), want_mixed)
        assert (exp['texts_split'], exp['texts_fallback']) == (4, 2)
        assert exp['segments'] == sum(n for n in n_seg if n)
        lead = 11
        flat = np.concatenate([np.full(lead, 3, np.int32)] + mixed)
        off = np.concatenate([[0], np.cumsum([len(t) for t in mixed])]).astype(np.int64) + lead
        enc.reset_split_stats()
        got, got_off = enc.encode_flat(flat, off)
        assert got_off.tolist() == np.concatenate([[0], np.cumsum([len(w) for w in want_mixed])]).tolist()
        assert got.tolist() == np.concatenate(want_mixed).tolist()
        assert enc.split_stats()['segments'] == exp['segments']
    finally:
        enc.close()


# ---- 2. a trained list over 40 ids ---------------------------------------------------------------

@pytest.mark.gpu
def test_trained_list_random_skewed_and_merged_ids():
    rng = np.random.default_rng(3)
    merges = trained_merges(rng, 40, 40, 300)
    lengths = [CAP + 1, 20000, 50000]
    vocab = 40 + len(merges)
    texts = random_texts(rng, 40, lengths) + skewed_texts(rng, 40, lengths) + random_texts(rng, vocab, lengths)
    enc = split_encoder(merges)
    try:
        exp = check_split(enc, texts, merges)
        assert exp['texts_fallback'] == 0 and exp['texts_split'] == len(texts)
    finally:
        enc.close()


# ---- 3. lists whose cut set is complete -------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize('alphabet', [3, 12])
def test_complete_cut_set_falls_back(alphabet):
    rng = np.random.default_rng({3: 1, 12: 2}[alphabet])      # (tests/test_encoder.py's lists)
    merges = trained_merges(rng, alphabet, 40, 300)
    _f, _l, keys = ends_and_cut_set(merges)
    assert len(keys) == alphabet * alphabet
    texts = random_texts(rng, alphabet, [CAP + 1, 100, 20000]) + skewed_texts(rng, alphabet, [CAP + 7])
    enc = split_encoder(merges)
    try:
        exp = check_split(enc, texts, merges)
        assert exp['texts_split'] == 0 and exp['texts_fallback'] == 3
    finally:
        enc.close()


# ---- 4. many segments ---------------------------------------------------------------------------------

@pytest.mark.gpu
def test_more_than_1024_segments():
    """More segments than one workgroup packs (k_scan_lens / k_gather) and than the few-texts
    form takes."""
    rng = np.random.default_rng(8)
    merges = fixture_a()
    lengths = [700 * H, 3, 324 * H + CAP + 1]
    assert sum(lengths) > 1024 * H + CAP
    texts = random_texts(rng, 9, lengths)                     # (an 8 every ninth token or so)
    enc = split_encoder(merges)
    try:
        exp = check_split(enc, texts, merges)
        assert exp['segments'] > 1024 and exp['texts_fallback'] == 0
    finally:
        enc.close()


# ---- 5. the tables follow the list --------------------------------------------------------------------

@pytest.mark.gpu
def test_tables_follow_add_merges_and_clear():
    merges = list(fixture_a())
    rng = np.random.default_rng(9)
    t0 = planted(rng, CAP + 1, [1])
    t0[2] = 0                                                 # 8 0: the boundary between them goes
    t1 = planted(rng, CAP + 1, [0])
    t1[1] = 0                                                 # its only safe boundary goes: falls back
    enc = split_encoder(merges)
    try:
        exp = check_split(enc, [t0, t1], merges)
        assert (exp['texts_split'], exp['segments']) == (2, 4)
        more = [(8, 0, 10 + len(merges))]
        enc.add_merges(more)
        merges2 = merges + more
        _e, plans_before = plan_stats([t0, t1], merges)
        exp, plans = plan_stats([t0, t1], merges2)
        assert plans_before[0] == [0, 2] and plans[0] == [0, 1] and plans[1] is None
        assert check_split(enc, [t0, t1], merges2) == exp
        enc.clear()
        fresh = trained_merges(np.random.default_rng(3), 40, 40, 300)
        enc.add_merges(fresh)
        exp = check_split(enc, random_texts(rng, 40, [CAP + 1, 30000]), fresh)
        assert exp['texts_split'] == 2
    finally:
        enc.close()


# ---- 6. opt-in only ------------------------------------------------------------------------------------

@pytest.mark.gpu
def test_the_route_is_opt_in(monkeypatch):
    texts, _n_seg, want = planted_with_reference()
    merges = fixture_a()
    monkeypatch.delenv('BPE_ENCODE_LONG', raising=False)
    enc = pkg.Encoder(0, merges)
    try:
        enc.reset_stats()
        got = enc.encode(texts[:2] + [np.zeros(5, np.int32)])
        assert [g.tolist() for g in got[:2]] == [w.tolist() for w in want[:2]]
        st, ss = enc.stats(), enc.split_stats()
        assert st['texts_replay'] == 2 and st['texts_rank'] == 1
        assert all(v == 0 for v in ss.values()), ss
        with pytest.raises(pkg.BpeError) as ei:
            enc.set_long_texts(7)
        assert ei.value.code == pkg.ERR_ARG
        enc.set_long_texts('split')
        check_split(enc, texts[:2], merges, want[:2])
        enc.set_long_texts('replay')
        enc.reset_stats()
        enc.encode(texts[:1])
        assert enc.stats()['texts_replay'] == 1
    finally:
        enc.close()
    monkeypatch.setenv('BPE_ENCODE_LONG', 'split')
    enc = pkg.Encoder(0, merges)
    try:
        exp = check_split(enc, texts[:2], merges, want[:2])
        assert exp['texts_split'] == 2
    finally:
        enc.close()


@pytest.mark.gpu
def test_lists_the_split_cannot_take_are_replayed():
    """A list the greedy cannot take (tests/test_encoder.py's) and one that makes an id twice: every
    long text is replayed in split mode, with no plan made."""
    rng = np.random.default_rng(10)
    not_greedy = [(0, 1, 2), (2, 0, 3), (1, 1, 0), (0, 2, 4)]
    twice = [(0, 1, 5), (2, 3, 5), (5, 4, 6)]
    for merges, alphabet in ((not_greedy, 3), (twice, 5)):
        assert not split_ok(merges)
        texts = random_texts(rng, alphabet, [CAP + 1, 300, 18000])
        enc = split_encoder(merges)
        try:
            exp = check_split(enc, texts, merges)
            assert exp['windows'] == 0 and enc.stats()['texts_replay'] >= 2
        finally:
            enc.close()


@pytest.mark.gpu
def test_bad_ids_in_long_texts_are_refused():
    """An id out of range never indexes a table: its boundaries are unsafe and the call fails with
    the bad-id error, on a text that splits and on one that falls back."""
    rng = np.random.default_rng(12)
    enc = split_encoder(fixture_a())
    try:
        for bad in (-3, pkg.MAX_VOCAB, 2 ** 31 - 1):
            t = planted(rng, CAP + 1, [1, 9000])
            t[12000] = bad
            with pytest.raises(pkg.BpeError, match='out of range'):
                enc.encode([t])
            t = planted(rng, CAP + 1, [])
            t[5] = bad
            with pytest.raises(pkg.BpeError, match='out of range'):
                enc.encode([t])
        texts, _n, want = planted_with_reference()
        check_split(enc, texts[:1], fixture_a(), want[:1])
    finally:
        enc.close()


# ---- CPU: the rule itself, and the package's names ------------------------------------------------------

def split_replay(text, merges, tables, h, cap):
    """The replays of the plan's segments, concatenated (None: the text falls back)."""
    starts = plan_text(text, tables, h, cap)
    if starts is None:
        return None
    edges = starts + [len(text)]
    parts = oracle.encode([text[a:b] for a, b in zip(edges, edges[1:])], merges)
    return np.concatenate(parts).tolist() if parts else []


def test_planted_segment_counts_cpu():
    """The plan of the six planted texts at the real caps: 2, 2, the window's count and 3 segments, two
    fallbacks."""
    tables = ends_and_cut_set(fixture_a())
    for t, n_seg in planted_cases(np.random.default_rng(5)):
        starts = plan_text(t, tables, H, CAP)
        assert (None if starts is None else len(starts)) == n_seg, len(t)
        if starts is not None:
            edges = starts + [len(t)]
            assert max(b - a for a, b in zip(edges, edges[1:])) <= CAP
    exact = plan_text(planted_cases(np.random.default_rng(5))[3][0], tables, H, CAP)
    assert exact == [0, CAP, CAP + 6]                         # (a segment of exactly CAP tokens)


def test_rule_on_planted_boundaries_cpu():
    """Fixture A at toy caps (H = 16, cap = 64): the same six shapes, and split + concatenate equal
    to the whole-text replay wherever the text splits."""
    h, cap = 16, 64
    merges = fixture_a()
    tables = ends_and_cut_set(merges)
    cases = planted_cases(np.random.default_rng(5), h, cap)
    want = oracle.encode([t for t, _n in cases], merges)
    assert sum(plan_text(t, tables, h, cap) is not None for t, _n in cases) >= 3
    for (t, _n_seg), w in zip(cases, want):
        starts = plan_text(t, tables, h, cap)
        if starts is not None:
            edges = starts + [len(t)]
            assert max(b - a for a, b in zip(edges, edges[1:])) <= cap
            assert split_replay(t, merges, tables, h, cap) == w.tolist()


@pytest.mark.parametrize('alphabet', [3, 12, 40])
def test_rule_on_trained_lists_cpu(alphabet):
    """Random, run-heavy and merged-id texts at toy caps: every text that splits equals its
    whole-text replay; the complete cut sets of alphabets 3 and 12 leave nothing to cut."""
    h, cap = 16, 64
    rng = np.random.default_rng({3: 1, 12: 2, 40: 3}[alphabet])
    merges = trained_merges(rng, alphabet, 40, 300)
    assert split_ok(merges)
    tables = ends_and_cut_set(merges)
    vocab = alphabet + len(merges)
    lengths = [cap, cap + 1, 100, 333, 1000, 2500]
    texts = random_texts(rng, alphabet, lengths) + skewed_texts(rng, alphabet, lengths) + \
        random_texts(rng, vocab, lengths)
    want = oracle.encode(texts, merges)
    n_split = 0
    for t, w in zip(texts, want):
        got = split_replay(t, merges, tables, h, cap)
        if got is not None:
            assert got == w.tolist(), len(t)
            n_split += len(t) > cap
    if alphabet == 40:
        assert n_split >= 10
    else:
        assert len(tables[2]) == alphabet * alphabet and n_split == 0


def test_package_exports_the_split_names():
    L = pkg.lib()
    for name in ('bpe_encoder_set_long_texts', 'bpe_encoder_get_split_stats', 'bpe_encoder_reset_split_stats'):
        assert name in pkg.C_API and hasattr(L, name)
    assert (pkg.LONG_REPLAY, pkg.LONG_SPLIT) == (0, 1)
    assert H & (H - 1) == 0 and 2 * H <= CAP
    assert ctypes.sizeof(pkg.SplitStats) == 48 and ctypes.sizeof(pkg.EncoderStats) == 56
    hdr = open(pkg.HERE + '/../include/bpe.h').read()
    assert '#define BPE_ENCODE_SPLIT_WINDOW %d ' % H in hdr
    assert '#define BPE_LONG_REPLAY 0\n' in hdr and '#define BPE_LONG_SPLIT 1\n' in hdr
    for name in ('set_long_texts', 'split_stats', 'reset_split_stats'):
        assert hasattr(pkg.Encoder, name)
