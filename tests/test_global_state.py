"""The sharded maintained state of the streaming mode (the "global state": bpe_set_global_counts,
rl_global in csrc/bpe_engine.hip, enter_maintained in csrc/bpe_multi.cpp) against a recount of the
oracle's corpus.  Every shard holds a copy of the GLOBAL hot bins and cold table; a merge
(a, b) -> c zeroes the pairs of a and b in every copy, each shard recounts the pairs with a side in
{a, b, c} on its own samples into delta rows of its exchange buffer, and the next selection adds
the rows, summed over the shards, to every copy.  Between two batches the last merge's rows still
wait in the exchange buffers: a copy then holds the recount of every pair with no side in
{a, b, c} and 0 for the others, and the rows, summed over the shards, hold the rest.

check_global() states that; its own tests (no GPU) build correct views in numpy, which must pass,
and corrupt them in one place at a time, which must fail with the message of that corruption.  The
GPU tests read every shard's tables and exchange buffer (Engine.maintained_tables(shard),
Engine.global_state(shard): they launch nothing and change nothing), drive the oracle alongside in
batches and compare with exact equality after every batch, once without reading the engine's
corpus between the batches and once with."""
import time

import numpy as np
import pytest

from bpe_amd import pkg
from oracle import OracleState
from test_digest_stream import flat
from test_maintained_state import (HOT, EMPTY, INCR_RLIM, TIES, block_maxima_corpus,
                                   hash_overflow_corpus, mixed_corpus, pair_count_arrays,
                                   pattern_corpus, random_cold_corpus, random_plan,
                                   rows_limit_corpus, transition_corpus)

gpu = pytest.mark.gpu

HDR = pkg.XCHG_HDR          # header words of the exchange buffer; word 0: the replacement count
ROWS = pkg.DELTA_ROWS       # (a, .) (b, .) (., a) (., b) (c, .) (., c), at HDR + ROWS * other + row
FORMS = ['tables', 'corpus']


# ---- the checker -----------------------------------------------------------------------------------
def delta_slot(x, y, a, b, c):
    """delta_slot of bpe_pass.hip.h on arrays: the one exchange word of the pair (x, y), by the
    first of x == a, x == b, y == a, y == b, x == c, (y == c) that holds."""
    x, y = np.asarray(x, np.int64), np.asarray(y, np.int64)
    conds = [x == a, x == b, y == a, y == b, x == c]
    row = np.select(conds, [0, 1, 2, 3, 4], 5)
    other = np.select(conds, [y, y, x, x, y], x)
    return HDR + ROWS * other + row


def row_pairs(words, a, b, c):
    """The pairs (x, y) that the words HDR + ROWS * other + row stand for."""
    i = np.asarray(words, np.int64) - HDR
    other, row = i // ROWS, i % ROWS
    m = np.array([a, b, a, b, c, c], np.int64)[row]
    left = (row == 0) | (row == 1) | (row == 4)
    return np.where(left, m, other), np.where(left, other, m), row, other


def _few(x, y, kept, want, n=8):
    return [(int(p), int(q), int(k), int(w)) for p, q, k, w in zip(x[:n], y[:n], kept[:n], want[:n])]


def _diff(got_k, got_c, want_k, want_c):
    """Keys (sorted, unique) and counts of two sparse tables: (keys, kept, want) where they differ."""
    allk = np.union1d(got_k, want_k)
    g = np.zeros(allk.size, np.int64)
    w = np.zeros(allk.size, np.int64)
    g[np.searchsorted(allk, got_k)] = got_c
    w[np.searchsorted(allk, want_k)] = want_c
    bad = g != w
    return allk[bad], g[bad], w[bad]


def check_global(views, want_keys, want_counts, last_merge):
    """Every shard's copy of the global state at rest (between two batches) against the recount
    (want_keys, want_counts) of the WHOLE corpus (pair_count_arrays).  views: per shard a dict of
    'hot', 'keys', 'counts' (Engine.maintained_tables(shard)) and 'state', 'xchg'
    (Engine.global_state(shard)); last_merge: (a, b, c, W) of the last merge the engine returned,
    c = tokens - 1.  With K the recount and T = {a, b, c} of the pending merge (empty when none is):

    State    Every shard reports the same state words; the state is held; a pending merge is
             last_merge; without one the merge words are -1.
    Hot      Every hot bin of a pair with no side in T equals K; every bin with a side in T is 0.
    Cold     No key is claimed twice (dead claims, count 0, included).  The live claims (a key, a
             count > 0) are exactly the cold pairs of K with no side in T, with K's counts; none
             has a side in T.
    Rows     Per shard: every word from HDR + ROWS * (c + 1) on is 0; every nonzero row word is
             its pair's own slot under delta_slot's precedence ((a, a) belongs to row 0, never to
             the (., a) row).  Summed over the shards the rows are K restricted to the pairs with
             a side in T, nothing missing, nothing extra.  Word 0 summed over the shards is W.
             Without a pending merge every word from HDR on is 0."""
    wk, wc = np.asarray(want_keys, np.int64), np.asarray(want_counts, np.int64)
    s0 = views[0]['state']
    for r, v in enumerate(views):
        assert v['state'] == s0, 'state words: shard %d reports %s, shard 0 %s' % (r, v['state'], s0)
    assert s0['held'], 'state words: the shards do not hold the global state (%s)' % s0
    kept = (s0['a'], s0['b'], s0['c'], s0['w'])
    if s0['pending']:
        assert last_merge is not None and kept == tuple(last_merge), (
            'state words: the pending merge (a, b, c, W) is %s, the last merge returned %s' % (kept, last_merge))
        a, b, c, W = kept
        T = np.array([a, b, c], np.int64)
    else:
        assert kept == (-1, -1, -1, -1), 'state words: no merge is pending, but (a, b, c, W) is %s' % (kept,)
        a = b = c = W = -1
        T = np.zeros(0, np.int64)
    wx, wy = wk >> 16, wk & 0xFFFF
    w_touched = np.isin(wx, T) | np.isin(wy, T)
    w_hot = (wx < HOT) & (wy < HOT)
    want_hot = np.zeros(pkg.HOT_BINS, np.int64)
    sel = w_hot & ~w_touched
    want_hot[wy[sel] * 256 + wx[sel]] = wc[sel]
    bins = np.arange(pkg.HOT_BINS)
    bin_touched = np.isin(bins & 255, T) | np.isin(bins >> 8, T)
    cold_k, cold_c = wk[~w_hot & ~w_touched], wc[~w_hot & ~w_touched]
    lim = HDR + ROWS * (c + 1)
    row_k, row_c = [], []
    header = 0
    for r, v in enumerate(views):
        # -- hot bins
        hot = v['hot'].astype(np.int64)
        assert hot.size == pkg.HOT_BINS
        bad = np.nonzero((hot != want_hot) & bin_touched)[0]
        assert bad.size == 0, ('shard %d: hot bins of the pending merge (%d, %d) -> %d not zeroed (a, b, kept, want)'
                               % (r, a, b, c), _few(bad & 255, bad >> 8, hot[bad], want_hot[bad]))
        bad = np.nonzero(hot != want_hot)[0]
        assert bad.size == 0, ('shard %d: hot bins (a, b, kept, want): %d differ' % (r, bad.size),
                               _few(bad & 255, bad >> 8, hot[bad], want_hot[bad]))
        # -- cold claims
        ck, cc = v['keys'].astype(np.int64), v['counts'].astype(np.int64)
        claimed = ck[ck != EMPTY]
        uniq, n_of = np.unique(claimed, return_counts=True)
        twice = uniq[n_of > 1]
        assert twice.size == 0, ('shard %d: cold keys claimed twice (a, b, times, -)' % r,
                                 _few(twice >> 16, twice & 0xFFFF, n_of[n_of > 1], n_of[n_of > 1]))
        live = (ck != EMPTY) & (cc > 0)
        order = np.argsort(ck[live], kind='stable')
        lk, lc = ck[live][order], cc[live][order]
        lx, ly = lk >> 16, lk & 0xFFFF
        of_c = (lx == c) | (ly == c)
        assert not of_c.any(), ('shard %d: cold claims of c = %d before its rows are added (a, b, kept, want)' % (r, c),
                                _few(lx[of_c], ly[of_c], lc[of_c], 0 * lc[of_c]))
        of_ab = np.isin(lx, T) | np.isin(ly, T)
        assert not of_ab.any(), ('shard %d: cold claims of the pending merge (%d, %d) not zeroed (a, b, kept, want)'
                                 % (r, a, b), _few(lx[of_ab], ly[of_ab], lc[of_ab], 0 * lc[of_ab]))
        dk, dg, dw = _diff(lk, lc, cold_k, cold_c)
        if dk.size:
            for what, m in (('cold pairs missing', dg == 0), ('cold claims of no pair of the corpus', dw == 0),
                            ('cold counts', (dg != 0) & (dw != 0))):
                assert not m.any(), ('shard %d: %s (a, b, kept, want): %d differ' % (r, what, int(m.sum())),
                                     _few(dk[m] >> 16, dk[m] & 0xFFFF, dg[m], dw[m]))
        # -- exchange rows
        x = v['xchg']
        assert x.size == pkg.XCHG_WORDS, 'shard %d: exchange buffer of %d words' % (r, x.size)
        if not s0['pending']:
            nz = np.nonzero(x[HDR:])[0] + HDR
            assert nz.size == 0, ('shard %d: exchange rows not zero while no merge is pending (word, value)' % r,
                                  [(int(i), int(x[i])) for i in nz[:8]])
            continue
        nz = np.nonzero(x[lim:])[0] + lim
        assert nz.size == 0, ('shard %d: exchange words past the rows of c = %d, from word %d on (word, value)'
                              % (r, c, lim), [(int(i), int(x[i])) for i in nz[:8]])
        nz = np.nonzero(x[HDR:lim])[0] + HDR
        px, py, row, other = row_pairs(nz, a, b, c)
        val = x[nz].astype(np.int64)
        bad = (row == 2) & (other == a)
        assert not bad.any(), ('shard %d: exchange rows: (a, a) = (%d, %d) belongs to row 0, not to the (., a) row '
                               '(word, value)' % (r, a, a), [(int(i), int(q)) for i, q in zip(nz[bad][:8], val[bad][:8])])
        own = delta_slot(px, py, a, b, c)
        bad = own != nz
        assert not bad.any(), ("shard %d: exchange rows: a count outside its pair's own slot (a, b, word, own slot)" % r,
                               _few(px[bad], py[bad], nz[bad], own[bad]))
        row_k.append((px << 16) | py)
        row_c.append(val)
        header += int(x[0])
    if not s0['pending']:
        return
    # -- the rows summed over the shards
    allk = np.concatenate(row_k)
    gk, inv = np.unique(allk, return_inverse=True)
    gc = np.bincount(inv, weights=np.concatenate(row_c).astype(np.float64), minlength=gk.size).astype(np.int64)
    dk, dg, dw = _diff(gk, gc, wk[w_touched], wc[w_touched])
    assert dk.size == 0, ('exchange rows summed over the %d shards against the recount of the pairs of (%d, %d) -> %d '
                          '(a, b, kept, want): %d differ' % (len(views), a, b, c, dk.size),
                          _few(dk >> 16, dk & 0xFFFF, dg, dw))
    assert header == W, "header: the shards' replacement counts (word 0) sum to %d, W = %d" % (header, W)


# ---- correct views in numpy, and single corruptions ------------------------------------------------
MODELS = {'hot': (0, 8, 0.0), 'cold': (300, 6, 0.0), 'mixed': (252, 8, 0.0), 'runs': (300, 5, 0.6)}   # first id, alphabet, runs


def model_views(name, pending=True, S=3):
    """A seeded small corpus over A ids from lo on (runs, an empty sample), the oracle's first
    merge applied, and S shards' views of it as the engine would hold them: the tables of every
    shard alike, dead claims (count 0) where pairs are gone or zeroed, holes, the touched pairs'
    counts split over the rows of shards 0 and 1; the last shard's rows all zero (a shard without
    samples).  pending=False: the rows added, the tables the whole recount."""
    lo, A, bias = MODELS[name]
    rng = np.random.default_rng(lo + A)
    samples = []
    for _ in range(5):
        runs = int(rng.integers(150, 400))
        toks = rng.integers(lo, lo + A, runs)
        lens = np.where(rng.random(runs) >= bias, 1, rng.integers(2, 7, runs))
        samples.append(np.repeat(toks, lens).astype(np.int32))
    samples.insert(2, np.zeros(0, np.int32))
    ids, off = flat(samples)
    st = OracleState(ids, off, [1] * (lo + A), lo + A, extra=64)
    bk, _ = pair_count_arrays(ids, off)
    (a, b, W), = st.merge_until(0, 2, 1)
    c = lo + A
    K = pair_count_arrays(st.ids[:st.off[-1]], st.off)
    wk, wc = K
    T = np.array([a, b, c] if pending else [], np.int64)
    x, y = wk >> 16, wk & 0xFFFF
    touched = np.isin(x, T) | np.isin(y, T)
    is_hot = (x < HOT) & (y < HOT)
    hot = np.zeros(pkg.HOT_BINS, np.uint64)
    sel = is_hot & ~touched
    hot[y[sel] * 256 + x[sel]] = wc[sel]
    sel = ~is_hot & ~touched
    gone = np.setdiff1d(bk[((bk >> 16) >= HOT) | ((bk & 0xFFFF) >= HOT)], wk[sel])    # dead claims
    keys = np.concatenate([wk[sel], gone, np.full(5, EMPTY)])
    counts = np.concatenate([wc[sel], np.zeros(gone.size + 5, np.int64)])
    order = rng.permutation(keys.size)
    keys, counts = keys[order].astype(np.uint32), counts[order].astype(np.uint64)
    rows = [np.zeros(pkg.XCHG_WORDS, np.uint64) for _ in range(S)]
    if pending:
        slot = delta_slot(x[touched], y[touched], a, b, c)
        assert np.unique(slot).size == slot.size
        part = rng.integers(0, wc[touched] + 1)
        rows[0][slot] = part
        rows[1][slot] = wc[touched] - part
        rows[0][0], rows[1][0] = W - W // 3, W // 3
    state = {'held': True, 'pending': pending, 'a': a if pending else -1, 'b': b if pending else -1,
             'c': c if pending else -1, 'w': W if pending else -1, 'multi_maintained': 1,
             'xchg_words': pkg.XCHG_WORDS}
    views = [{'hot': hot.copy(), 'keys': keys.copy(), 'counts': counts.copy(), 'state': dict(state),
              'xchg': rows[r]} for r in range(S)]
    return views, K, (a, b, c, W), rng


@pytest.mark.parametrize('pending', [True, False])
@pytest.mark.parametrize('name', list(MODELS))
def test_checker_accepts_correct_views(name, pending):
    views, (wk, wc), last, _ = model_views(name, pending)
    check_global(views, wk, wc, last)
    a, b, c, W = last
    assert (a == b) == (name == 'runs')                     # (one model's merge is (a, a))
    if name == 'hot':
        assert c < HOT and views[0]['keys'].size == 5       # (c is hot: its row and column are bins)
    if name == 'cold':
        assert not views[0]['hot'].any()
    if pending:
        # the model has what the corruptions below need: pairs among a, b and c, rows on two
        # shards and none on the third, dead claims of a or b
        x, y = wk >> 16, wk & 0xFFFF
        assert (np.isin(x, [a, b, c]) & np.isin(y, [a, b, c])).any()
        assert views[0]['xchg'][HDR:].any() and views[1]['xchg'][HDR:].any() and not views[2]['xchg'].any()
        assert sum(int(v['xchg'][0]) for v in views) == W
    else:
        assert not any(v['xchg'].any() for v in views)


def _untouched_hot_bin(views, last):
    a, b, c, _ = last
    hot = views[0]['hot']
    i = np.nonzero(hot)[0]
    i = i[~np.isin(i & 255, [a, b, c]) & ~np.isin(i >> 8, [a, b, c])]
    return int(i[len(i) // 2])


def _live(v):
    return np.nonzero((v['keys'] != EMPTY) & (v['counts'] > 0))[0]


def _hole(v):
    return int(np.nonzero(v['keys'] == EMPTY)[0][0])


def c_hot_bin(delta):
    def f(views, last, rng):
        i = _untouched_hot_bin(views, last)
        for v in views:                                     # (all the shards wrong alike)
            v['hot'][i] = int(v['hot'][i]) + delta
    return f


def c_cold_count(delta):
    def f(views, last, rng):
        v = views[1]
        i = _live(v)
        i = int(i[v['counts'][i] >= 2][0])
        v['counts'][i] = int(v['counts'][i]) + delta
    return f


def c_key_twice(views, last, rng):
    v = views[0]
    v['keys'][_hole(v)] = v['keys'][_live(v)[0]]            # (a dead claim of a live key)


def c_claim_missing(views, last, rng):
    v = views[2]
    v['counts'][_live(v)[3]] = 0


def c_claim_extra(views, last, rng):
    v = views[0]
    i = _hole(v)
    v['keys'][i] = ((last[2] + 5) << 16) | (last[2] + 9)
    v['counts'][i] = 4


def c_claim_of_a_kept(views, last, rng):
    v = views[1]
    dead = np.nonzero((v['keys'] != EMPTY) & (v['counts'] == 0) & ((v['keys'] >> 16) == last[0]))[0]
    v['counts'][dead[0]] = 3


def c_hot_bin_of_b_kept(views, last, rng):
    a, b, c, _ = last
    assert b < HOT
    y = next(t for t in range(8) if t not in (a, b, c))
    views[0]['hot'][y * 256 + b] = 5


def c_claim_of_c(views, last, rng):
    v = views[0]
    i = _hole(v)
    v['keys'][i] = (last[2] << 16) | 301
    v['counts'][i] = 2


def c_row_to_a_lower_slot(views, last, rng):
    a, b, c, _ = last
    x = views[0]['xchg']
    nz = np.nonzero(x[HDR:])[0] + HDR
    px, py, row, other = row_pairs(nz, a, b, c)
    for i, p, q in zip(nz.tolist(), px.tolist(), py.tolist()):
        slots = [HDR + ROWS * o + r for r, (m, o) in enumerate([(p == a, q), (p == b, q), (q == a, p), (q == b, p),
                                                                  (p == c, q), (q == c, p)]) if m]
        assert slots[0] == i
        if len(slots) > 1 and not (p == q == a):
            x[slots[1]], x[i] = x[i], 0
            return
    raise AssertionError('the model has no pair among a, b and c in shard 0')


def c_aa_in_the_row_of_a(views, last, rng):
    views[2]['xchg'][HDR + ROWS * last[0] + 2] = 1


def c_row_count(delta):
    def f(views, last, rng):
        x = views[1]['xchg']
        i = np.nonzero(x[HDR:])[0] + HDR
        i = int(i[len(i) // 2])
        x[i] = int(x[i]) + delta
    return f


def c_word_past_the_rows(views, last, rng):
    views[2]['xchg'][HDR + ROWS * (last[2] + 1) + 3] = 1


def c_last_word(views, last, rng):
    views[0]['xchg'][pkg.XCHG_WORDS - 1] = 7


def c_header(views, last, rng):
    views[0]['xchg'][0] += np.uint64(1)


def c_one_shards_hot(views, last, rng):
    views[2]['hot'][_untouched_hot_bin(views, last)] += np.uint64(1)


def c_another_merge(views, last, rng):
    views[1]['state']['b'] += 1


def c_not_held(views, last, rng):
    for v in views:
        v['state']['held'] = False


def c_row_while_not_pending(views, last, rng):
    views[1]['xchg'][HDR + 17] = 1


CORRUPTIONS = [   # name, model, pending, corruption, the message it must fail with
    ('hot_bin_plus_1', 'hot', True, c_hot_bin(1), 'shard 0: hot bins (a, b, kept, want)'),
    ('hot_bin_minus_1', 'mixed', True, c_hot_bin(-1), 'shard 0: hot bins (a, b, kept, want)'),
    ('cold_count_plus_1', 'cold', True, c_cold_count(1), 'shard 1: cold counts'),
    ('cold_count_minus_1', 'mixed', True, c_cold_count(-1), 'shard 1: cold counts'),
    ('key_claimed_twice', 'cold', True, c_key_twice, 'shard 0: cold keys claimed twice'),
    ('live_claim_missing', 'cold', True, c_claim_missing, 'shard 2: cold pairs missing'),
    ('extra_live_claim', 'cold', True, c_claim_extra, 'shard 0: cold claims of no pair of the corpus'),
    ('claim_of_a_not_zeroed', 'cold', True, c_claim_of_a_kept, 'shard 1: cold claims of the pending merge'),
    ('hot_bin_of_b_not_zeroed', 'hot', True, c_hot_bin_of_b_kept, 'shard 0: hot bins of the pending merge'),
    ('claim_with_a_side_c', 'cold', True, c_claim_of_c, 'shard 0: cold claims of c'),
    ('row_word_in_a_lower_slot', 'cold', True, c_row_to_a_lower_slot, "shard 0: exchange rows: a count outside its pair's own slot"),
    ('row_word_in_a_lower_slot_hot', 'hot', True, c_row_to_a_lower_slot, "shard 0: exchange rows: a count outside its pair's own slot"),
    ('row_word_in_a_lower_slot_merge_a_a', 'runs', True, c_row_to_a_lower_slot, "shard 0: exchange rows: a count outside its pair's own slot"),
    ('a_a_in_the_row_of_a', 'cold', True, c_aa_in_the_row_of_a, 'shard 2: exchange rows: (a, a)'),
    ('row_count_plus_1', 'cold', True, c_row_count(1), 'exchange rows summed over the 3 shards'),
    ('row_count_minus_1', 'mixed', True, c_row_count(-1), 'exchange rows summed over the 3 shards'),
    ('word_past_the_rows', 'cold', True, c_word_past_the_rows, 'shard 2: exchange words past the rows'),
    ('last_word_of_the_buffer', 'hot', True, c_last_word, 'shard 0: exchange words past the rows'),
    ('header_sum', 'cold', True, c_header, 'header:'),
    ('one_shards_hot_table', 'mixed', True, c_one_shards_hot, 'shard 2: hot bins (a, b, kept, want)'),
    ('another_pending_merge', 'cold', True, c_another_merge, 'state words: shard 1 reports'),
    ('state_not_held', 'cold', True, c_not_held, 'state words: the shards do not hold'),
    ('hot_bin_not_pending', 'hot', False, c_hot_bin(1), 'shard 0: hot bins (a, b, kept, want)'),
    ('cold_count_not_pending', 'cold', False, c_cold_count(-1), 'shard 1: cold counts'),
    ('row_word_not_pending', 'cold', False, c_row_while_not_pending, 'shard 1: exchange rows not zero while no merge is pending'),
]


@pytest.mark.parametrize('name,model,pending,corrupt,message', CORRUPTIONS, ids=[c[0] for c in CORRUPTIONS])
def test_checker_rejects_a_single_corruption(name, model, pending, corrupt, message):
    views, (wk, wc), last, rng = model_views(model, pending)
    corrupt(views, last, rng)
    with pytest.raises(AssertionError) as err:
        check_global(views, wk, wc, last)
    assert message in str(err.value), str(err.value)[:400]


def test_checker_rejects_another_last_merge():
    views, (wk, wc), (a, b, c, W), _ = model_views('cold')
    for other in [(a, b, c, W + 1), (a, b, c + 1, W), (a + 1, b, c, W), (a, b + 1, c, W), None]:
        with pytest.raises(AssertionError) as err:
            check_global(views, wk, wc, other)
        assert 'state words: the pending merge' in str(err.value)


def test_delta_slot_restated():
    """delta_slot's precedence on the pairs among a, b and c (bpe_pass.hip.h), and row_pairs as its
    inverse on every row."""
    a, b, c = 7, 3, 11
    word = lambda other, row: HDR + ROWS * other + row
    for (x, y), want in {(a, 5): word(5, 0), (b, 5): word(5, 1), (5, a): word(5, 2), (5, b): word(5, 3),
                         (c, 5): word(5, 4), (5, c): word(5, 5), (a, a): word(a, 0), (a, b): word(b, 0),
                         (b, a): word(a, 1), (b, b): word(b, 1), (a, c): word(c, 0), (c, a): word(c, 2),
                         (b, c): word(c, 1), (c, b): word(c, 3), (c, c): word(c, 4)}.items():
        assert int(delta_slot(x, y, a, b, c)) == want, (x, y)
        px, py, _, _ = row_pairs([want], a, b, c)
        assert (int(px[0]), int(py[0])) == (x, y)
    assert int(delta_slot(a, a, a, a, c)) == word(a, 0)          # the merge (a, a)


def test_accessors_refuse_null_arguments():
    import ctypes
    L = pkg.lib()
    n = ctypes.c_int64(7)
    info = (ctypes.c_int64 * len(pkg.GLOBAL_INFO))(*([7] * len(pkg.GLOBAL_INFO)))
    hot = np.zeros(pkg.HOT_BINS, np.uint64)
    assert L.bpe_debug_tables_shard(None, 0, hot.ctypes.data, None, None, 0, ctypes.byref(n)) == pkg.ERR_ARG
    assert L.bpe_debug_global(None, -1, info, None, 0) == pkg.ERR_ARG
    assert n.value == 7 and list(info) == [7] * len(pkg.GLOBAL_INFO)


def test_rank_heavy_list_retry_leaves_room_and_gives_up():
    """GpuShard.heavy (sharded.py), the rank processes' form of find_next_merge_host's retry: the
    list's length counts the claims that lost a race, so the pass again may list a few more than
    the pass that sized the buffers.  A stub engine on CPU tensors: the second pass lists three
    more and must fit; a list that outgrows its buffers every time is an error after three."""
    import importlib
    import torch
    sharded = importlib.import_module('bpe-tokenizer_amd.sharded')

    class Stub:
        def __init__(self, lengths):
            self.lengths, self.caps = list(lengths), []

        def heavy_counts(self, table, keys, counts, cap, max_length):
            self.caps.append(cap)
            return self.lengths.pop(0)(cap)

    def shard(engine):
        s = sharded.GpuShard.__new__(sharded.GpuShard)
        s.engine, s.torch, s.device, s.cap = engine, torch, torch.device('cpu'), 1 << 16
        s.keys = torch.zeros(s.cap, dtype=torch.int32)
        s.counts = torch.zeros(s.cap, dtype=torch.int64)
        return s

    table = torch.zeros(8, dtype=torch.int64)
    n0 = 1 << 17                                    # (a power of two: no room by rounding alone)
    e = Stub([lambda cap: n0, lambda cap: n0 + 3])
    keys, counts = shard(e).heavy(table, 0)
    assert e.caps == [1 << 16, 1 << 18] and len(keys) == len(counts) == n0 + 3
    e = Stub([lambda cap: cap + 1] * 4)
    with pytest.raises(RuntimeError):
        shard(e).heavy(table, 0)
    assert len(e.caps) == 4 and not e.lengths
    assert shard(Stub([lambda cap: -1])).heavy(table, 0) is None


# ---- the corpora -------------------------------------------------------------------------------------
def cut_at_fillers(sample, k, fillers, lo=0):
    """One sample cut into k, each cut right behind a filler token (so that no planted site, a run
    of other tokens, is split), the nearest such place to j / k of the sample and not before lo."""
    s = np.asarray(sample)
    ok = np.nonzero(np.isin(s[:-1], fillers))[0] + 1
    ok = ok[ok >= max(lo, 1)]
    cuts = [int(ok[np.argmin(np.abs(ok - (lo + (len(s) - lo) * j // k)))]) for j in range(1, k)]
    assert cuts == sorted(set(cuts)), cuts
    return [p.astype(np.int32) for p in np.split(s, cuts)]


def cut_patterns(V, k):
    (s,), len16, planted = pattern_corpus(V)
    return cut_at_fillers(s, k, np.arange(HOT, HOT + 24)), len16, planted


def cut_rows_limit():
    (s,), len16, planted = rows_limit_corpus()
    used = {300, 301, 310, 311, 312, 313, *range(INCR_RLIM - 2, INCR_RLIM + 8)}
    fillers = np.array([i for i in range(HOT, INCR_RLIM - 2) if i not in used])
    return cut_at_fillers(s, 2, fillers), len16, planted


def cut_hash_overflow():
    """(the a b y_i block, the first 6000 tokens, whole in the first sample)"""
    (s,), len16, ab = hash_overflow_corpus()
    parts = cut_at_fillers(s, 2, np.arange(400, 2400), lo=6000)
    assert len(parts[0]) > 6000
    return parts, len16, ab


def compaction_corpus():
    """test_compaction_between_maintained_batches' corpus as two samples of 1.1 M tokens, the
    45 000 planted sites in the first only: of two shards the first compacts (its third merge
    kills more than 1 % of its slots) with delta rows pending, the second does not."""
    rng = np.random.default_rng(14)
    buf = rng.integers(HOT, HOT + 60, size=1_100_000).astype(np.int32)
    ids6 = [HOT + 60 + i for i in range(6)]
    p, q, r_, s, h1, h2 = ids6
    sites = [(p, q)] * 16_000 + [(r_, s)] * 15_000 + [(h1, h2)] * 14_000
    cells = rng.permutation(len(buf) // 4 - 2)[:len(sites)] + 1
    for (x, y), cell in zip(sites, cells):
        buf[4 * cell + 1:4 * cell + 3] = [x, y]
    other = rng.integers(HOT, HOT + 60, size=1_100_000).astype(np.int32)
    return [buf, other], [1] * (HOT + 66), [(p, q), (r_, s), (h1, h2)]


def oracle_merges(samples, len16, n):
    ids, off = flat(samples)
    return OracleState(ids, off, len16, len(len16), extra=1024).merge_until(0, 2, n)


@pytest.mark.parametrize('V,k', [(320, 4), (321, 4), (INCR_RLIM + 8, 2)])
def test_cut_pattern_corpora_keep_their_planted_merges(V, k):
    """(the oracle alone) pattern_corpus cut into k samples: the same planted winners."""
    samples, len16, planted = cut_patterns(V, k)
    assert len(samples) == k and all(len(s) > 100 for s in samples)
    got = [m[:2] for m in oracle_merges(samples, len16, 24)]
    assert got[:2] == planted[:2], got[:2]
    for pair in planted[2:]:
        assert pair in got[2:], (pair, got)


def test_cut_placed_corpora_keep_their_planted_merges():
    """(the oracle alone) the rows' limit, the hash overflow and the compaction corpora as cut here."""
    samples, len16, planted = cut_rows_limit()
    got = [m[:2] for m in oracle_merges(samples, len16, 16)]
    assert got[:3] == planted[:3] and planted[3] in got, got
    samples, len16, ab = cut_hash_overflow()
    assert oracle_merges(samples, len16, 3)[2] == ab + (2000,)
    samples, len16, planted = compaction_corpus()
    assert [m[:2] for m in oracle_merges(samples, len16, 3)] == planted
    assert not np.isin(samples[1], np.array(planted).ravel()).any()


# ---- the driver --------------------------------------------------------------------------------------
class Trajectory:
    """The oracle's side of a case, computed once and shared by the case's two forms: the steps
    (merge batches, added samples) in order, each with the merges, the corpus and its recount
    after it.  A replay must ask for the same steps."""
    last = (None, None)

    @classmethod
    def of(cls, key, samples, len16):
        if cls.last[0] != key:
            cls.last = (key, cls(samples, len16))       # (only the latest case's is kept)
        return cls.last[1]

    def __init__(self, samples, len16):
        ids, off = flat(samples)
        self.st = OracleState(ids, off, len16, len(len16), extra=1024)
        self.steps = []

    def step(self, i, op, fn):
        if i == len(self.steps):
            out = fn(self.st)
            ids, off = self.st.ids[:self.st.off[-1]].copy(), self.st.off.copy()
            self.steps.append((op, out, ids, off, pair_count_arrays(ids, off)))
        assert self.steps[i][0] == op, (i, self.steps[i][0], op)
        return self.steps[i][1:]


def shard_view(e, r=None):
    hot, keys, counts = e.maintained_tables(shard=r)
    state, xchg = e.global_state(shard=r)
    return {'hot': hot, 'keys': keys, 'counts': counts, 'state': state, 'xchg': xchg}


class GlobalRun:
    """pkg.Engine(devices=[0] * S, reduce='host') and the oracle side by side.  batch(): one
    merge_until on both, equal merges, then check(): in the form 'corpus' the engine's corpus
    equals the oracle's first; then, if every shard reports the global state, check_global on all
    the shards against the recount of the oracle's corpus.  held: per check point whether the
    state was held (and so checked).  Some shards holding the state and others not is a failure
    at once: the next batch's exchange sizes would differ."""

    def __init__(self, key, samples, len16, S, form, devices=None, reduce='host', mode=None):
        self.S, self.form = S, form
        self.tr = Trajectory.of(key, samples, len16)
        self.e = pkg.Engine(devices=devices or [0] * S, reduce=reduce)
        for i, l in enumerate(len16):
            self.e.set_token_len16(i, l)
        for s in samples:
            self.e.add_sample(s)
        if mode:
            self.e.set_mode(mode)
        self.e.stats_enable(True)
        self.i = 0
        self.merges = []
        self.held = []
        self.short = []             # the check points after a batch that ran out of pairs
        self.pending = 0
        self.t0 = time.perf_counter()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.e.close()

    def oracle(self, op, fn):
        out = self.tr.step(self.i, op, fn)
        self.i += 1
        self.ids, self.off, self.counts = out[1:]
        return out[0]

    def compare_corpus(self):
        ids, off = self.e.read_corpus()
        assert off.tolist() == self.off.tolist()
        assert np.array_equal(ids, self.ids)

    def check(self, read=None):
        if self.form == 'corpus' if read is None else read:
            self.compare_corpus()
        views = [shard_view(self.e, r) for r in range(self.S)]
        held = [v['state']['held'] for v in views]
        assert all(held) or not any(held), ('some shards hold the global state, some do not', held)
        self.held.append(held[0])
        if held[0]:
            a, b, W = self.merges[-1]
            try:
                check_global(views, *self.counts, (a, b, self.e.num_tokens() - 1, W))
            except AssertionError as x:
                raise AssertionError('check point %d, after %d merges (%s): %s' % (
                    len(self.held), len(self.merges), self.merges[-1], x))
            self.pending += views[0]['state']['pending']

    def batch(self, max_length, n, read=None):
        w = self.oracle(('merge', max_length, n), lambda st: st.merge_until(max_length, 2, n))
        got = self.e.merge_until(max_length, 2, n)
        assert got == w, (len(self.merges), got[:3], w[:3])
        self.merges += w
        self.check(read)
        if len(w) < n:
            self.short.append(len(self.held))       # (no pair left under this max_length)
        return len(w)

    def finish(self, name, missed=(), late=False):
        """The corpus at the end; the condition on every case: the state was held at every check
        point but the first and those in `missed` (1-based: the check points a planted hand-off
        or transition may cost), and at two or more (at one, where only one batch ran to its end)."""
        self.compare_corpus()
        stats = self.e.stats()
        print('%s [%s] S=%d: %d merges, %d check points, held %s, %d pending, %.2f s; %s' % (
            name, self.form, self.S, len(self.merges), len(self.held), ''.join('x' if h else '-' for h in self.held),
            self.pending, time.perf_counter() - self.t0,
            {k: stats[k] for k in ('loop_host', 'fused_passes', 'exact_passes', 'compactions', 'pix_merges')}))
        lost = [i + 1 for i, h in enumerate(self.held) if not h]
        if late and any(self.held):
            # (a corpus of hot ids starts in the table state and enters this one when its cold
            # pairs outgrow the sketch: the check points before that, and none after it)
            lost = [i for i in lost if i > self.held.index(True)]
        assert set(lost) <= {1, *missed}, ('the global state was not held at check points', lost, self.held)
        # (a batch that ran out of pairs leaves the state by design, and a corpus merged to its end
        # inside its first batch has one check point that can hold it)
        full = len(self.held) - len(self.short)
        assert sum(self.held) >= max(1, min(2, full)), (
            'the global state was reached at fewer than two check points', self.held, self.short)
        return stats


FORM = pytest.mark.parametrize('form', FORMS)


# ---- a. random, all cold -----------------------------------------------------------------------------
# The two host iterations that enter the state each end a call of one merge: with bs = 1 the state
# is first held at the third check point (bpe_multi.cpp: heavy_streak >= 2), otherwise at the first.
# A batch that runs out of pairs under its max_length ends without its last iteration merging, so
# every shard leaves the state (rank_loop_end) and the next batch enters it again: such a batch
# costs its own check point, and with bs = 1 the two after it.
@gpu
@FORM
@pytest.mark.parametrize('bs', [1, 8, 40])
@pytest.mark.parametrize('seed,S', [(0, 2), (0, 3), (1, 2), (1, 3), (3, 2), (3, 3)],
                         ids=['seed0_S2_one_shard_empty', 'seed0_S3_two_shards_empty', 'seed1_S2', 'seed1_S3',
                              'seed3_S2', 'seed3_S3'])
def test_random_all_cold(seed, S, bs, form):
    samples, len16, merges, rng = random_cold_corpus(seed)
    if bs == 1:
        merges = min(merges, 40)
    with GlobalRun(('random', seed, bs), samples, len16, S, form) as r:
        for max_length, n in random_plan(rng, merges, bs):
            if len(r.merges) >= merges:
                break
            r.batch(max_length, n)
        assert len(r.merges) >= min(merges, 40), len(r.merges)
        missed = {i + k for i in r.short for k in range(3 if bs == 1 else 1)} | ({2} if bs == 1 else set())
        r.finish('random seed %d bs %d' % (seed, bs), missed=missed)
        if bs == 1:
            # (every merge's rows were seen, but those of the iterations that enter the state)
            assert r.pending >= len(r.merges) - len(missed) - 1, (r.pending, len(r.merges), sorted(missed))


# ---- b. hot and cold sides ---------------------------------------------------------------------------
@gpu
@FORM
def test_mixed_hot_and_cold(form):
    samples, len16 = mixed_corpus()
    with GlobalRun('mixed', samples, len16, 3, form) as r:
        for _ in range(10):
            r.batch(0, 8)
        ab = np.array([m[:2] for m in r.merges])
        assert (ab < HOT).any() and (ab >= HOT).any(), 'corpus: merges on one side of 256 only'
        r.finish('mixed')


# ---- c. pairs among a, b and c -----------------------------------------------------------------------
@gpu
@FORM
@pytest.mark.parametrize('S', [2, 4])
@pytest.mark.parametrize('V', [320, 321])
def test_pairs_among_a_b_and_c(V, S, form):
    samples, len16, planted = cut_patterns(V, 4)
    with GlobalRun(('patterns', V), samples, len16, S, form) as r:
        for _ in range(24):
            r.batch(0, 1)
        got = [m[:2] for m in r.merges]
        assert got[:2] == planted[:2], got[:2]
        for pair in planted[2:]:
            assert pair in got[2:], (pair, got)
        r.finish('patterns V %d' % V, missed=(2,))
        # every planted merge after the two that enter was checked with its rows pending
        assert all(r.held[2:]), r.held


# ---- d. past the rows' limit -------------------------------------------------------------------------
@gpu
@FORM
@pytest.mark.parametrize('which', ['neighbours', 'vocabulary'])
def test_past_the_rows_limit(which, form):
    """A multi-device context leaves the streaming mode by itself at 18 432 ids: set_mode('stream')
    keeps it, and no merge may have run on a position index."""
    samples, len16, planted = cut_rows_limit() if which == 'neighbours' else cut_patterns(INCR_RLIM + 8, 2)
    with GlobalRun(('rows_limit', which), samples, len16, 2, form, mode='stream') as r:
        # 'neighbours': after its four planted merges the corpus has only ties of more than
        # BPE_MAX_CAND pairs at W = 6, which the device hands to the host, where a multi-device
        # context leaves the state.  So the third planted merge (its neighbours on both sides of
        # the limit) and the fourth (its own tokens past it) each end a batch, and the batch of 8
        # behind them may end outside the state.
        for n in ([3, 1, 8] if which == 'neighbours' else [8, 8, 8]):
            r.batch(0, n)
        got = [m[:2] for m in r.merges]
        assert got[:2] == planted[:2] and all(p in got for p in planted), got
        stats = r.finish('rows limit ' + which, missed=(3,) if which == 'neighbours' else ())
        assert r.held[:2] == [True, True], r.held
        assert stats['pix_merges'] == 0, stats


# ---- e. the LDS hash's overflow into the delta sink ----------------------------------------------------
@gpu
@FORM
def test_lds_hash_overflows_to_the_delta_rows(form):
    samples, len16, ab = cut_hash_overflow()
    with GlobalRun('hash_overflow', samples, len16, 2, form) as r:
        r.batch(0, 8)
        r.batch(0, 8)
        assert r.merges[2] == ab + (2000,), r.merges[:3]
        r.finish('hash overflow')
        assert all(r.held), r.held


# ---- f. block maxima, ties and hand-off ----------------------------------------------------------------
@gpu
@FORM
@pytest.mark.parametrize('bs', [40, 64])
def test_block_maxima_ties_and_hand_off(bs, form):
    """The tie groups of 17 and 40 pairs exceed BPE_MAX_CAND: the device hands those iterations to
    the host protocol, every shard leaves the state, one host iteration later the shards enter it
    again (enter_maintained: one exact pass per shard) and the batch goes on.  The hand-offs fall
    inside the calls, so every check point sees the state as re-entered."""
    samples, len16 = block_maxima_corpus()
    total = 12 + sum(n for n, _ in TIES) + 5
    S = 2
    with GlobalRun(('block_maxima', bs), samples, len16, S, form) as r:
        # (three batches: 64 merges end inside the group of 40, whose hand-offs may cost the first
        # check point)
        for _ in range(3):
            r.batch(0, bs)
        assert len(r.merges) >= total
        W = [m[2] for m in r.merges[:12]]
        assert W == sorted(W, reverse=True) and W[0] == 400 and W[11] == 295, r.merges[:12]
        at = 12
        for n, w in TIES:
            assert all(m[2] == w for m in r.merges[at:at + n]), (n, w, r.merges[at:at + n])
            at += n
        stats = r.finish('block maxima bs %d' % bs)
        # Left and re-entered.  Every shard counts every hand-over (loop_host sums over the
        # shards).  Entering takes two: every id here is >= 256, so every pair is a sketch pair,
        # the table state's first iteration already needs exact cold counts and is handed over,
        # and so is the second; no merge is made in the table state.  A third hand-over per shard
        # is one after the entry, where every shard leaves the state (rank_loop_end).
        assert stats['loop_host'] >= 3 * S, stats
        # The same from the merges: each one made in the state is one fused pass on every shard,
        # the others were made by the host protocol, two to enter and the handed-over ones.  The
        # state is held, and exact, at the check point after it was entered again.
        assert stats['fused_passes'] % S == 0, stats
        by_host = len(r.merges) - stats['fused_passes'] // S
        assert by_host >= 3 and r.held[-1], (by_host, r.held, stats)


# ---- g. compaction inside the state ----------------------------------------------------------------------
@gpu
@FORM
def test_compaction_with_delta_rows_pending(form):
    samples, len16, planted = compaction_corpus()
    with GlobalRun('compaction', samples, len16, 2, form) as r:
        for max_length, n in [(0, 3), (0, 8), (0, 8)]:
            r.batch(max_length, n)
        assert [m[:2] for m in r.merges[:3]] == planted, r.merges[:3]
        stats = r.finish('compaction')
        assert stats['compactions'] >= 1, stats
        assert r.held[-2:] == [True, True], r.held


# ---- h. transitions ----------------------------------------------------------------------------------------
def t_add_sample(r):
    new = r.ids[100:700].copy()
    r.e.add_sample(new)

    def add(st):
        st.ids = np.concatenate([st.ids[:st.off[-1]], new])
        st.off = np.concatenate([st.off, [st.off[-1] + len(new)]]).astype(np.int64)
    r.oracle(('add', len(new)), add)
    r.check()


def t_host_merge(r):
    (a, b, W), = w = r.oracle(('merge', 0, 1), lambda st: st.merge_until(0, 2, 1))
    assert r.e.find_next_merge(0, 2) == (a, b, W)
    assert r.e.apply_merge(a, b, r.e.num_tokens()) == W
    r.merges += w
    r.check()


def t_index_merge(r):
    w = r.oracle(('merge', 0, 1), lambda st: st.merge_until(0, 2, 1))
    r.e.set_mode('incremental')
    assert r.e.merge_until(0, 2, 1) == w
    r.e.set_mode('stream')
    r.merges += w
    r.check()


def t_read(r):
    r.compare_corpus()
    assert r.e.sample_lengths().tolist() == np.diff(r.off).tolist()
    r.oracle(('read',), lambda st: None)
    r.check()


TRANSITIONS = {'add_sample': t_add_sample, 'host_merge': t_host_merge, 'index_merge': t_index_merge,
               'read': t_read}


@gpu
@FORM
@pytest.mark.parametrize('name', list(TRANSITIONS))
def test_transition_between_batches(name, form):
    """Each transition keeps every shard's tables exact or makes every shard drop the state
    (check() tells which, and checks the tables if they are kept); after the next batches the
    state is held again and exact."""
    samples, len16 = transition_corpus()
    with GlobalRun(('transition', name), samples, len16, 2, form) as r:
        r.batch(0, 8)
        assert r.held[-1], 'the state was not entered'
        TRANSITIONS[name](r)                    # check point 2
        kept = r.held[-1]
        r.batch(0, 8)                           # 3: (re-entry takes two host iterations inside the batch)
        assert r.held[-1], ('no re-entry', r.held)
        TRANSITIONS[name](r)                    # 4
        r.batch(0, 8)
        r.batch(0, 8)
        print(name, 'kept' if kept else 'dropped')
        r.finish('transition ' + name, missed=(2, 4))
        assert r.held[-2:] == [True, True], r.held


# ---- i. a realistic mix --------------------------------------------------------------------------------------
@gpu
@FORM
def test_zipf_words_over_three_shards(form):
    data = pkg.synth_zipf(2 << 20, seed=12345)
    chars, first = np.unique(data, return_index=True)
    cmap = np.zeros(256, np.int32)
    cmap[chars[np.argsort(first)]] = np.arange(chars.size)      # ids by first appearance
    nt = int(chars.size)
    samples = np.split(cmap[data], np.arange(1 << 18, 2 << 20, 1 << 18))
    assert len(samples) == 8
    with GlobalRun('zipf', samples, [1] * nt, 3, form) as r:
        for _ in range(8):
            r.batch(0, 64)
        assert len(r.merges) == 512
        r.finish('zipf words', late=True)


# ---- j. RCCL on one device -------------------------------------------------------------------------------------
@gpu
@FORM
def test_rccl_one_device_context(form):
    """S = 1 with the real all-reduce (ncclCommInitAll over [0]) on the shard's stream."""
    samples, len16, merges, rng = random_cold_corpus(3)
    with GlobalRun(('random', 3, 8), samples, len16, 1, form, devices=[0], reduce='rccl') as r:
        for max_length, n in random_plan(rng, merges, 8):
            if len(r.merges) >= merges:
                break
            r.batch(max_length, n)
        r.finish('rccl one device')


# ---- the accessors' refusals on the device -------------------------------------------------------------------------
@gpu
def test_accessors_refuse_bad_contexts_shards_and_buffers():
    import ctypes
    L = pkg.lib()
    n = ctypes.c_int64()
    info = (ctypes.c_int64 * len(pkg.GLOBAL_INFO))()
    hot = np.zeros(pkg.HOT_BINS, np.uint64)
    one = pkg.Engine(0)
    multi = pkg.Engine(devices=[0, 0], reduce='host')
    try:
        # a single context: no shard's tables; its own global state only as shard -1
        assert L.bpe_debug_tables_shard(one._ctx, 0, hot.ctypes.data, None, None, 0, ctypes.byref(n)) == pkg.ERR_ARG
        assert L.bpe_debug_global(one._ctx, 0, info, None, 0) == pkg.ERR_ARG
        assert L.bpe_debug_global(one._ctx, -1, None, None, 0) == pkg.ERR_ARG
        state, xchg = one.global_state()
        assert state == {'held': False, 'pending': False, 'a': -1, 'b': -1, 'c': -1, 'w': -1,
                         'multi_maintained': -1, 'xchg_words': 0} and xchg.size == 0
        for shard in (-1, 2):
            assert L.bpe_debug_tables_shard(multi._ctx, shard, hot.ctypes.data, None, None, 0,
                                            ctypes.byref(n)) == pkg.ERR_ARG
            assert L.bpe_debug_global(multi._ctx, shard, info, None, 0) == pkg.ERR_ARG
        assert L.bpe_debug_tables_shard(multi._ctx, 0, None, None, None, 0, ctypes.byref(n)) == pkg.ERR_ARG
        assert L.bpe_debug_tables_shard(multi._ctx, 0, hot.ctypes.data, None, None, 0, None) == pkg.ERR_ARG
        assert L.bpe_debug_tables_shard(multi._ctx, 0, hot.ctypes.data, None, None, 4, ctypes.byref(n)) == pkg.ERR_ARG
        assert L.bpe_debug_global(multi._ctx, 0, None, None, 0) == pkg.ERR_ARG
        assert L.bpe_debug_global(multi._ctx, 0, info, None, 4) == pkg.ERR_ARG
        # a fresh multi-device context holds nothing
        for shard in (0, 1):
            state, xchg = multi.global_state(shard)
            assert not state['held'] and not state['pending'] and state['multi_maintained'] == 0 and xchg.size == 0
            assert multi.maintained_tables(shard)[1].size == 0
    finally:
        one.close()
        multi.close()
