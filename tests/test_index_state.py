"""The state of the position index (the incremental mode, csrc/bpe_pix.hip.h) against a recount of
the oracle's corpus: not only the merges it selects, but every count, list, link and maximum it
keeps, after the build, after every merge, at batch boundaries, after the pool and the table grow,
after a hand-off's rebuild and in every shard of a sharded corpus.  check_index() states the
invariants; its own tests (no GPU) build a correct view in numpy, which must pass, and corrupt it
in one place at a time, which must fail with the message of that corruption.  The GPU tests read
the live index through Engine.pix_view() from the hook of bpe_debug_pix_hook (a single context
keeps its index only inside merge_until) or between the calls (a shard keeps it), drive the oracle
alongside and compare with exact equality throughout."""
import time

import numpy as np
import pytest

from bpe_amd import make_engine, pkg
from oracle import OracleState
from test_digest_stream import flat
from test_maintained_state import pair_count_arrays

gpu = pytest.mark.gpu

NONE = 0xFFFFFFFF           # PIX_NONE: no slot (links), an empty table key
SEP = -1                    # between samples; anything below it is a merged-away slot (TOMB)
PIX_B = 256                 # table slots per block
PIX_SB = 256                # blocks per superblock
PIX_PROBE = 4096            # longest probe sequence
HOT = 256                   # a pair of two ids below it is counted in LDS by the build


# ---- the checker -----------------------------------------------------------------------------------
def pix_hash(key):
    """pix_hash of bpe_pix.hip.h on an int64 array of keys."""
    h = (np.asarray(key, np.int64) * 0x9E3779B1) & 0xFFFFFFFF
    return h ^ (h >> 15)


def sel_of(keys, cnt, len16, ml):
    """pix_sel_of: the packed selection key W << 17 | 0x1FFFF - (u + v) of every table slot, 0 for
    an empty slot, a count of 0 and a pair whose UTF-16 lengths sum past max_length (ml > 0)."""
    keys = np.asarray(keys, np.int64)
    cnt = np.asarray(cnt).astype(np.int64)
    u, v = keys >> 16, keys & 0xFFFF
    ok = (keys != NONE) & (cnt > 0)
    if ml > 0:
        l16 = np.zeros(1 << 16, np.int64)
        l16[:min(len(len16), 1 << 16)] = np.asarray(len16[:1 << 16], np.int64)
        ok &= l16[u] + l16[v] <= ml
    return np.where(ok, (cnt << 17) | (0x1FFFF - (u + v)), 0)


def pair_of(key):
    return int(key) >> 16, int(key) & 0xFFFF


def check_index(view, ids, off, len16, ml, counts=None, n_built=0):
    """Every invariant of a position index at rest (between two merges), as the code keeps them.
    view: Engine.pix_view(); ids, off: the corpus the index is over (a shard: its own samples);
    counts: (keys, counts) the table must hold when that is not the recount of ids, off (a shard:
    the global recount); n_built: the token ids that existed when the index was built.

    Corpus   The live slots (tok >= SEP) in slot order are the corpus, every sample followed by one
             SEP.  nxt / prv link ALL live slots, separators included, each to the next / previous
             live slot (the build links i to i +- 1, a merge unlinks only the slot it kills); the
             ends are PIX_NONE; no merged-away slot is linked from a live one.
    Table    No key twice; every key within PIX_PROBE probes of pix_hash(key) & mask with no empty
             slot before it; `used` counts every claim alike (the build's hot and cold claims,
             k_pix_alloc's owner entries, a shard's pix_global_add): used == claimed keys, and
             used <= used_cap.
    Counts   cnt of every pair of the recount equals it (a run of L equal tokens counts L // 2),
             whatever max_length filters; every other claimed key has 0; every pair has a key.
    Lists    Segments (len > 0) lie in [0, pool_top), pool_top <= pool_cap, and are disjoint.  fill
             == len for every list written through its fill counter: the cold pairs of the build
             and every pair a merge made; the build writes its hot pairs' lists (both ids < 256 and
             < n_built) through LDS cursors and leaves fill at 0.  No position twice in a list.
             For EVERY pair (u, v), u == v included, the entries p with tok[p] == u and
             tok[nxt[p]] == v are exactly the positions where u is followed by v: the build lists
             every position of an (x, x) run, odd offsets too (only the count skips them), and a
             merge lists every (c, c) adjacency it makes, so k_pix_sites finds each run by its head
             and the tie scan's last valid entry is the run's last adjacency.
    Maxima   bmax[b] == max of pix_sel_of over block b.  A single context recomputes the blocks a
             merge marked in the same merge (k_pix_alloc), so there bdirty is 0 everywhere; a shard
             recomputes them at the start of the next iteration (k_pix_dirty), so between batches
             bdirty is set for exactly the blocks dblocks lists, and those alone may be too high.
             sbmax[s] == max of the kept bmax of its blocks, except the superblocks dsuper lists,
             which may be too high only (the next k_pix_select recomputes them before it reads
             any); sbdirty is set for exactly those."""
    v = view
    n, cap = v['n'], v['cap']
    tok = v['tok'].astype(np.int64)
    nxt, prv = v['nxt'].astype(np.int64), v['prv'].astype(np.int64)
    keys = v['keys'].astype(np.int64)
    cnt = v['cnt'].astype(np.int64)
    toff, tlen, tfill = v['off'].astype(np.int64), v['len'].astype(np.int64), v['fill'].astype(np.int64)
    pool = v['pool'].astype(np.int64)
    sharded = bool(v['sharded'])
    assert v['status'] in (pkg.PIX_RUN, pkg.PIX_PAUSE, pkg.PIX_DONE), ('status', v['status'], v['err'])
    assert v['ml'] == ml, ('max_length of the index', v['ml'], ml)
    assert cap > 0 and cap & (cap - 1) == 0 and v['nblocks'] == cap // PIX_B, ('capacity', cap, v['nblocks'])
    assert v['nsuper'] == (v['nblocks'] + PIX_SB - 1) // PIX_SB, ('superblocks', v['nsuper'])
    mask = cap - 1

    # -- corpus
    ids = np.asarray(ids, np.int64)
    off = np.asarray(off, np.int64)
    want_tok = np.full(ids.size + off.size - 1, SEP, np.int64)
    dst = np.arange(ids.size) + np.searchsorted(off[1:], np.arange(ids.size), side='right')
    want_tok[dst] = ids
    live = np.nonzero(tok >= SEP)[0]
    if live.size != want_tok.size or not np.array_equal(tok[live], want_tok):
        k = min(live.size, want_tok.size)
        bad = np.nonzero(tok[live[:k]] != want_tok[:k])[0]
        i = int(bad[0]) if bad.size else k
        raise AssertionError('corpus: %d live slots, want %d; live slot %d (slot %d) holds %s, want %s' % (
            live.size, want_tok.size, i, int(live[i]) if i < live.size else -1,
            int(tok[live[i]]) if i < live.size else None, int(want_tok[i]) if i < want_tok.size else None))
    want_nxt = np.append(live[1:], NONE)
    want_prv = np.append(NONE, live[:-1])
    bad = np.nonzero(nxt[live] != want_nxt)[0]
    assert bad.size == 0, 'links: nxt[%d] = %d, want %d' % (live[bad[0]], nxt[live[bad[0]]], want_nxt[bad[0]])
    bad = np.nonzero(prv[live] != want_prv)[0]
    assert bad.size == 0, 'links: prv[%d] = %d, want %d' % (live[bad[0]], prv[live[bad[0]]], want_prv[bad[0]])

    # -- table
    slots = np.nonzero(keys != NONE)[0]
    ck = keys[slots]
    order = np.argsort(ck, kind='stable')
    sk, ss = ck[order], slots[order]
    dup = np.nonzero(sk[1:] == sk[:-1])[0]
    assert dup.size == 0, 'table: key (%d, %d) claimed twice (slots %d and %d)' % (
        pair_of(sk[dup[0]]) + (ss[dup[0]], ss[dup[0] + 1]))
    home = pix_hash(ck) & mask
    dist = (slots - home) & mask
    empties = np.concatenate([[0], np.cumsum(keys == NONE)])        # empties[i]: empty slots below i
    between = np.where(home <= slots, empties[slots] - empties[home],
                       empties[cap] - empties[home] + empties[slots])
    bad = np.nonzero((between != 0) | (dist >= PIX_PROBE))[0]
    assert bad.size == 0, 'table: key (%d, %d) at slot %d is behind an empty slot of its probe sequence (home %d)' % (
        pair_of(ck[bad[0]]) + (slots[bad[0]], home[bad[0]]))
    assert v['used'] == slots.size, 'table: used = %d, claimed keys = %d' % (v['used'], slots.size)
    assert v['used'] <= v['used_cap'], 'table: used = %d past used_cap = %d' % (v['used'], v['used_cap'])

    # -- counts
    wk, wc = pair_count_arrays(ids, off) if counts is None else counts
    wk, wc = np.asarray(wk, np.int64), np.asarray(wc, np.int64)
    at = np.searchsorted(sk, wk)
    found = (at < sk.size) & (sk[np.minimum(at, sk.size - 1)] == wk) if sk.size else np.zeros(wk.size, bool)
    bad = np.nonzero(~found)[0]
    assert bad.size == 0, 'counts: pair (%d, %d) of the corpus has no key (want %d)' % (
        pair_of(wk[bad[0]]) + (wc[bad[0]],))
    want_cnt = np.zeros(cap, np.int64)
    want_cnt[ss[at]] = wc
    bad = np.nonzero(cnt[slots] != want_cnt[slots])[0]
    assert bad.size == 0, 'counts: pair (%d, %d) kept %d, want %d (%d pairs differ)' % (
        pair_of(ck[bad[0]]) + (cnt[slots[bad[0]]], want_cnt[slots[bad[0]]], bad.size))

    # -- lists
    top = v['pool_top']
    assert top <= v['pool_cap'], 'lists: pool_top = %d past pool_cap = %d' % (top, v['pool_cap'])
    assert pool.size == top
    ls = slots[tlen[slots] > 0]
    bad = np.nonzero(toff[ls] + tlen[ls] > top)[0]
    assert bad.size == 0, 'lists: segment of (%d, %d) [%d, %d) outside the pool [0, %d)' % (
        pair_of(keys[ls[bad[0]]]) + (toff[ls[bad[0]]], toff[ls[bad[0]]] + tlen[ls[bad[0]]], top))
    o = np.argsort(toff[ls], kind='stable')
    lo = ls[o]
    bad = np.nonzero(toff[lo[:-1]] + tlen[lo[:-1]] > toff[lo[1:]])[0]
    assert bad.size == 0, 'lists: segments of (%d, %d) [%d, %d) and (%d, %d) [%d, ..) overlap' % (
        pair_of(keys[lo[bad[0]]]) + (toff[lo[bad[0]]], toff[lo[bad[0]]] + tlen[lo[bad[0]]]) +
        pair_of(keys[lo[bad[0] + 1]]) + (toff[lo[bad[0] + 1]],))
    lu, lv = keys[ls] >> 16, keys[ls] & 0xFFFF
    built_hot = (lu < min(HOT, n_built)) & (lv < min(HOT, n_built))
    want_fill = np.where(built_hot, 0, tlen[ls])
    bad = np.nonzero(tfill[ls] != want_fill)[0]
    assert bad.size == 0, 'lists: fill of (%d, %d) = %d, len = %d (want fill %d)' % (
        pair_of(keys[ls[bad[0]]]) + (tfill[ls[bad[0]]], tlen[ls[bad[0]]], want_fill[bad[0]]))
    e_slot = np.repeat(lo, tlen[lo])
    start = np.cumsum(tlen[lo]) - tlen[lo]
    e_at = toff[e_slot] + (np.arange(e_slot.size) - np.repeat(start, tlen[lo]))
    p = pool[e_at]
    bad = np.nonzero(p >= n)[0]
    assert bad.size == 0, 'lists: entry %d of (%d, %d) is no slot (n = %d)' % (
        (p[bad[0]],) + pair_of(keys[e_slot[bad[0]]]) + (n,))
    e_key = keys[e_slot]
    tagged = np.sort((e_slot << 32) | p)
    dup = np.nonzero(tagged[1:] == tagged[:-1])[0]
    assert dup.size == 0, 'lists: position %d twice in the list of (%d, %d)' % (
        (tagged[dup[0]] & 0xFFFFFFFF,) + pair_of(keys[tagged[dup[0]] >> 32]))
    q = nxt[p]
    qs = np.where(q == NONE, 0, q)
    valid = (tok[p] == (e_key >> 16)) & (q != NONE) & (tok[qs] == (e_key & 0xFFFF))
    got = np.sort((e_key[valid] << 32) | p[valid])
    lp = live[:-1][(want_tok[:-1] >= 0) & (want_tok[1:] >= 0)]     # a token followed by a token
    want = np.sort((((tok[lp] << 16) | tok[nxt[lp]]) << 32) | lp)
    if not np.array_equal(got, want):
        miss = np.setdiff1d(want, got)
        extra = np.setdiff1d(got, want)
        x = int(miss[0]) if miss.size else int(extra[0])
        raise AssertionError('lists: position %d of (%d, %d) is %s (%d missing, %d unexpected)' % (
            (x & 0xFFFFFFFF,) + pair_of(x >> 32) +
            ('in the corpus but not in its list' if miss.size else 'in its list but not in the corpus',
             miss.size, extra.size)))

    # -- maxima
    sel = sel_of(keys, cnt, len16, ml)
    want_b = sel.reshape(v['nblocks'], PIX_B).max(axis=1)
    bmax = v['bmax'].astype(np.int64)
    listed_b = np.zeros(v['nblocks'], bool)
    if sharded:
        assert (v['dblocks'] < v['nblocks']).all(), ('maxima: dblocks names no block', v['dblocks'][:8])
        listed_b[v['dblocks']] = True
    bad = np.nonzero((bmax != want_b) & ~listed_b)[0]
    if bad.size:
        b = int(bad[0])
        s = b * PIX_B + int(np.argmax(sel[b * PIX_B:(b + 1) * PIX_B]))
        raise AssertionError('maxima: bmax[%d] = %d is too %s, want %d (W %d of (%d, %d) at slot %d; %d blocks differ)' % (
            (b, bmax[b], 'high' if bmax[b] > want_b[b] else 'low', want_b[b], want_b[b] >> 17) +
            pair_of(keys[s]) + (s, bad.size)))
    bad = np.nonzero(bmax < want_b)[0]
    assert bad.size == 0, 'maxima: bmax[%d] = %d of a listed block is too low, want %d' % (
        bad[0] if bad.size else 0, bmax[bad[0]] if bad.size else 0, want_b[bad[0]] if bad.size else 0)
    bad = np.nonzero((v['bdirty'] != 0) != listed_b)[0]
    assert bad.size == 0, 'maxima: bdirty[%d] = %d, listed %s' % (bad[0], v['bdirty'][bad[0]], listed_b[bad[0]])
    pad = np.zeros(v['nsuper'] * PIX_SB, np.int64)
    pad[:v['nblocks']] = bmax
    want_s = pad.reshape(v['nsuper'], PIX_SB).max(axis=1)
    sbmax = v['sbmax'].astype(np.int64)
    listed_s = np.zeros(v['nsuper'], bool)
    assert (v['dsuper'] < v['nsuper']).all(), ('maxima: dsuper names no superblock', v['dsuper'][:8])
    listed_s[v['dsuper']] = True
    bad = np.nonzero((sbmax != want_s) & ~listed_s)[0]
    assert bad.size == 0, 'maxima: sbmax[%d] = %d is too %s, want %d' % (
        bad[0], sbmax[bad[0]], 'high' if sbmax[bad[0]] > want_s[bad[0]] else 'low', want_s[bad[0]])
    bad = np.nonzero(sbmax < want_s)[0]
    assert bad.size == 0, 'maxima: sbmax[%d] = %d of a listed superblock is too low, want %d' % (
        bad[0], sbmax[bad[0]], want_s[bad[0]])
    bad = np.nonzero((v['sbdirty'] != 0) != listed_s)[0]
    assert bad.size == 0, 'maxima: sbdirty[%d] = %d, listed %s' % (bad[0], v['sbdirty'][bad[0]], listed_s[bad[0]])
    if v['tie'] == pkg.PIX_TIE_DECIDED:
        # a tie scanned and decided, not committed: the pair it names holds the best key
        s = v['pair_slot']
        assert s < cap and keys[s] != NONE and sel[s] == sel.max() and sel[s] > 0, (
            'tie: the decided pair at slot %d does not hold the best key' % s)


# ---- a correct view in numpy, and single corruptions -------------------------------------------------
def model_view(seed, A, ml, cap_log2=12, tombs=0.15, stale=0.2, dead_keys=20):
    """A seeded small corpus over A ids (runs, empty and one-token samples) laid out as an index at
    rest would hold it: merged-away slots between the tokens, every pair's positions in a pool
    segment with stale entries among them, claimed keys whose pairs are gone, exact maxima.  Ids
    from `n_built` on count as made by merges (their lists were written through fill)."""
    rng = np.random.default_rng(seed)
    samples = []
    for _ in range(int(rng.integers(2, 9))):
        kind = rng.random()
        if kind < 0.15:
            samples.append(np.zeros(0, np.int32))
        elif kind < 0.3:
            samples.append(rng.integers(0, A, 1).astype(np.int32))
        else:
            runs = int(rng.integers(1, 150))
            toks = rng.integers(0, A, runs)
            lens = np.where(rng.random(runs) < 0.6, 1, rng.integers(2, 9, runs))
            samples.append(np.repeat(toks, lens).astype(np.int32))
    samples.append(np.array([0, 0, 0, 1, 1, 0, 1, 0, 1], np.int32))
    ids, off = flat(samples)
    len16 = rng.integers(1, 3, A).tolist()
    n_built = max(2, A - A // 4)
    dense = np.concatenate([np.append(s, SEP) for s in samples]).astype(np.int64)
    # merged-away slots after some of the slots (never slot 0: a merge kills the right slot)
    gaps = np.where(rng.random(dense.size) < tombs, rng.integers(1, 4, dense.size), 0)
    pos = np.arange(dense.size) + np.concatenate([[0], np.cumsum(gaps)[:-1]])
    n = int(pos[-1] + 1 + gaps[-1])
    tok = np.full(n, -2, np.int64)
    tok[pos] = dense
    nxt = rng.integers(0, n, n)          # (a dead slot's links are whatever they were)
    prv = rng.integers(0, n, n)
    nxt[pos] = np.append(pos[1:], NONE)
    prv[pos] = np.append(NONE, pos[:-1])
    cap = 1 << cap_log2
    keys = np.full(cap, NONE, np.int64)
    cnt = np.zeros(cap, np.int64)
    toff = rng.integers(0, 1 << 30, cap)  # (never written for a pair without a list)
    tlen = np.zeros(cap, np.int64)
    tfill = rng.integers(0, 1 << 30, cap)

    def claim(key):
        s = int(pix_hash(key)) & (cap - 1)
        while keys[s] != NONE:
            assert keys[s] != key
            s = (s + 1) & (cap - 1)
        keys[s] = key
        return s

    adj = np.nonzero((dense[:-1] >= 0) & (dense[1:] >= 0))[0]
    akey = (dense[adj] << 16) | dense[adj + 1]
    wk, wc = pair_count_arrays(ids, off)
    pool = []
    for key in rng.permutation(np.unique(akey)):
        s = claim(int(key))
        cnt[s] = wc[np.searchsorted(wk, key)]
        mine = pos[adj[akey == key]]
        others = np.setdiff1d(pos, mine)
        entries = np.concatenate([mine, rng.choice(others, int(stale * mine.size) + (rng.random() < stale),
                                                   replace=False)])
        entries = rng.permutation(entries)
        toff[s], tlen[s] = len(pool), entries.size
        u, w = int(key) >> 16, int(key) & 0xFFFF
        tfill[s] = 0 if u < min(HOT, n_built) and w < min(HOT, n_built) else entries.size
        pool.extend(entries.tolist())
    for _ in range(dead_keys):            # pairs that are gone: a key, count 0, a stale list or none
        key = int(rng.integers(0, A)) << 16 | int(rng.integers(A, A + 50))
        if key in keys:
            continue
        s = claim(key)
        if rng.random() < 0.5:
            entries = rng.choice(pos, 3, replace=False)
            toff[s], tlen[s], tfill[s] = len(pool), 3, 3
            pool.extend(entries.tolist())
    nblocks = cap // PIX_B
    nsuper = (nblocks + PIX_SB - 1) // PIX_SB
    sel = sel_of(keys, cnt, len16, ml)
    bmax = sel.reshape(nblocks, PIX_B).max(axis=1)
    pad = np.zeros(nsuper * PIX_SB, np.int64)
    pad[:nblocks] = bmax
    view = {
        'present': 1, 'n': n, 'cap': cap, 'nblocks': nblocks, 'nsuper': nsuper, 'ml': ml,
        'status': pkg.PIX_RUN, 'tie': pkg.PIX_TIE_NONE, 'err': 0, 'used': int((keys != NONE).sum()),
        'used_cap': cap // 10 * 7, 'pool_top': len(pool), 'pool_cap': len(pool) + 64, 'n_dblocks': 0,
        'n_dsuper': 0, 'next_id': A, 'merged': 0, 'n_done': 0, 'sharded': 0, 'delta_pending': 0,
        'pair_slot': 0, 'max_id': 55296,
        'tok': tok.astype(np.int32), 'nxt': nxt.astype(np.uint32), 'prv': prv.astype(np.uint32),
        'keys': keys.astype(np.uint32), 'cnt': cnt.astype(np.uint64), 'off': toff.astype(np.uint32),
        'len': tlen.astype(np.uint32), 'fill': tfill.astype(np.uint32), 'bmax': bmax.astype(np.uint64),
        'sbmax': pad.reshape(nsuper, PIX_SB).max(axis=1).astype(np.uint64),
        'bdirty': np.zeros(nblocks, np.uint32), 'sbdirty': np.zeros(nsuper, np.uint32),
        'pool': np.array(pool, np.uint32), 'dblocks': np.zeros(0, np.uint32), 'dsuper': np.zeros(0, np.uint32),
    }
    return view, (ids, off, len16, ml), n_built


MODELS = [(seed, A, ml, cap) for seed, (A, cap) in enumerate([(2, 10), (3, 12), (7, 12), (30, 12), (300, 13), (40, 17)])
          for ml in (0, 3)]


def check_model(view, corpus, n_built):
    check_index(view, *corpus, n_built=n_built)


@pytest.mark.parametrize('seed,A,ml,cap', MODELS)
def test_checker_accepts_a_correct_view(seed, A, ml, cap):
    view, corpus, n_built = model_view(seed, A, ml, cap)
    check_model(view, corpus, n_built)
    assert (view['tok'] < SEP).any() and view['pool_top'] > 0
    # what may lawfully be stale passes too: a superblock listed as dirty whose max is too high
    view['sbmax'][0] += 1 << 17
    view['sbdirty'][0] = 1
    view['dsuper'] = np.array([0], np.uint32)
    view['n_dsuper'] = 1
    check_model(view, corpus, n_built)
    # ... and a shard's listed block (recomputed by the next iteration's k_pix_dirty)
    view['sharded'] = 1
    b = int(np.argmax(view['bmax']))
    view['bmax'][b] += 1 << 17
    view['bdirty'][b] = 1
    view['dblocks'] = np.array([b], np.uint32)
    view['n_dblocks'] = 1
    view['sbmax'][0] = max(view['sbmax'][0], view['bmax'][b])
    check_model(view, corpus, n_built)


def _slots_with_lists(v, least=2):
    return np.nonzero((v['keys'] != NONE) & (v['len'] >= least))[0]


def _valid_entries(v, s):
    """Indices into the pool of the still-valid entries of slot s."""
    u, w = pair_of(v['keys'][s])
    out = []
    for i in range(int(v['off'][s]), int(v['off'][s] + v['len'][s])):
        p = int(v['pool'][i])
        q = int(v['nxt'][p])
        if v['tok'][p] == u and q != NONE and v['tok'][q] == w:
            out.append(i)
    return out


def _not_the_max(v, corpus):
    """A slot with a list and a count that is neither the global maximum nor its block's."""
    sel = sel_of(v['keys'], v['cnt'], corpus[2], corpus[3])
    for s in _slots_with_lists(v, 1):
        if v['cnt'][s] > 0 and sel[s] < v['bmax'][s // PIX_B] and _valid_entries(v, s):
            return int(s)
    return None


def c_count(delta):
    def f(v, corpus, rng):
        s = _not_the_max(v, corpus)
        if s is None:                      # (every pair is its block's max: any pair then)
            s = int(_slots_with_lists(v, 1)[0])
        c = int(v['cnt'][s]) + delta
        v['cnt'][s] = c
        if c == 0 or sel_of(v['keys'], v['cnt'], corpus[2], corpus[3])[s] > v['bmax'][s // PIX_B]:
            v['cnt'][s] = c + 2           # (stay a count fault, not a maxima fault)
    return f


def c_drop_entry(v, corpus, rng):
    for s in _slots_with_lists(v):
        ve = _valid_entries(v, s)
        if ve:
            stale = [p for p in range(v['n']) if v['tok'][p] == SEP]
            v['pool'][ve[0]] = stale[0]    # (the entry now names a separator: stale for every pair)
            return
    raise AssertionError('no list to corrupt')


def c_move_entry(v, corpus, rng):
    """A valid entry leaves its list for the list next to it in the pool: it becomes the last entry
    of its own segment, and the boundary between the two segments moves one entry to the left."""
    order = sorted(_slots_with_lists(v, 2), key=lambda s: int(v['off'][s]))
    for s, t in zip(order, order[1:]):
        ve = _valid_entries(v, s)
        end = int(v['off'][s] + v['len'][s])
        if not ve or end != v['off'][t] or v['pool'][ve[0]] in v['pool'][end:end + v['len'][t]]:
            continue
        v['pool'][ve[0]], v['pool'][end - 1] = v['pool'][end - 1], v['pool'][ve[0]]
        for name in ('len', 'fill'):
            if name == 'len' or v['fill'][s]:
                v[name][s] -= 1
            if name == 'len' or v['fill'][t]:
                v[name][t] += 1
        v['off'][t] -= 1
        return
    raise AssertionError('no two neighbouring lists to corrupt')


def c_dup_key(v, corpus, rng):
    s = int(_slots_with_lists(v, 1)[0])
    t = (s + 1) & (v['cap'] - 1)
    while v['keys'][t] != NONE:
        t = (t + 1) & (v['cap'] - 1)
    v['keys'][t] = v['keys'][s]
    v['cnt'][t] = 0
    v['len'][t] = 0
    v['used'] += 1


def c_key_behind_empty(v, corpus, rng):
    """A key moved past the empty slot that ends its probe sequence."""
    s = int(_slots_with_lists(v, 1)[0])
    t = s
    while v['keys'][t] != NONE:
        t = (t + 1) & (v['cap'] - 1)
    t = (t + 1) & (v['cap'] - 1)
    while v['keys'][t] != NONE:
        t = (t + 1) & (v['cap'] - 1)
    for name in ('keys', 'cnt', 'off', 'len', 'fill'):
        v[name][t] = v[name][s]
    v['keys'][s] = NONE
    # (the maxima follow the move: this is a table fault alone)
    sel = sel_of(v['keys'], v['cnt'], corpus[2], corpus[3])
    v['bmax'][:] = sel.reshape(v['nblocks'], PIX_B).max(axis=1)


def c_bmax(delta):
    def f(v, corpus, rng):
        b = int(np.argmax(v['bmax']))
        if delta > 0:
            b = int(np.argmin(v['bmax']))   # (a block below its superblock's max: sbmax stays right)
            if v['nblocks'] == 1 or v['bmax'][b] + (1 << 17) > v['bmax'].max():
                v['sbmax'][b // PIX_SB] = max(v['sbmax'][b // PIX_SB], v['bmax'][b] + np.uint64(1 << 17))
            v['bmax'][b] += np.uint64(1 << 17)
        else:
            v['bmax'][b] -= np.uint64(1 << 17)
            pad = np.zeros(v['nsuper'] * PIX_SB, np.uint64)
            pad[:v['nblocks']] = v['bmax']
            v['sbmax'][:] = pad.reshape(v['nsuper'], PIX_SB).max(axis=1)
    return f


def c_sbmax_low(v, corpus, rng):
    v['sbmax'][int(np.argmax(v['sbmax']))] -= np.uint64(1 << 17)


def c_prv(v, corpus, rng):
    live = np.nonzero(v['tok'] >= SEP)[0]
    i = int(live[len(live) // 2])
    v['prv'][i] = live[len(live) // 2 - 2]


def c_overlap(v, corpus, rng):
    order = sorted(_slots_with_lists(v, 2), key=lambda s: int(v['off'][s]))
    s, t = order[0], order[1]
    # t's segment starts inside s's (its content moves with it)
    seg = v['pool'][v['off'][t]:v['off'][t] + v['len'][t]].copy()
    v['off'][t] = v['off'][s] + v['len'][s] - 1
    keep = v['pool'][v['off'][s] + v['len'][s] - 1]
    v['pool'][v['off'][t]:v['off'][t] + v['len'][t]] = seg
    v['pool'][v['off'][t]] = keep


def c_fill(v, corpus, rng):
    for s in _slots_with_lists(v, 1):
        if v['fill'][s] == v['len'][s]:
            v['fill'][s] -= 1
            return
    raise AssertionError('no list written through fill')


CORRUPTIONS = [
    ('count_plus_1', c_count(1), r'counts: pair .* kept \d+, want \d+'),
    ('count_minus_1', c_count(-1), r'counts: pair .* kept \d+, want \d+'),
    ('dropped_entry', c_drop_entry, r'lists: position \d+ of .* is in the corpus but not in its list'),
    ('moved_entry', c_move_entry, r'lists: position \d+ of .* is in the corpus but not in its list'),
    ('duplicated_key', c_dup_key, r'table: key .* claimed twice'),
    ('key_behind_empty', c_key_behind_empty, r'table: key .* is behind an empty slot'),
    ('bmax_low', c_bmax(-1), r'maxima: bmax\[\d+\] = \d+ is too low'),
    ('bmax_high', c_bmax(1), r'maxima: bmax\[\d+\] = \d+ is too high'),
    ('sbmax_low', c_sbmax_low, r'maxima: sbmax\[\d+\] = \d+ is too low'),
    ('broken_prv', c_prv, r'links: prv\[\d+\] = \d+, want \d+'),
    ('overlap', c_overlap, r'lists: segments of .* overlap'),
    ('fill_ne_len', c_fill, r'lists: fill of .* = \d+, len = \d+'),
]


@pytest.mark.parametrize('name,corrupt,message', CORRUPTIONS, ids=[c[0] for c in CORRUPTIONS])
def test_checker_rejects_a_single_corruption(name, corrupt, message):
    """Each corruption of a correct view alone, on every model: rejected, with its own message."""
    for seed, A, ml, cap in MODELS:
        view, corpus, n_built = model_view(seed, A, ml, cap)
        corrupt(view, corpus, np.random.default_rng(seed))
        with pytest.raises(AssertionError, match=message):
            check_model(view, corpus, n_built)


def test_pix_hash_and_selection_key_restated():
    """The two restated formulas on values worked out by hand from bpe_pix.hip.h."""
    assert int(pix_hash(np.array([1]))[0]) == 0x9E3779B1 ^ (0x9E3779B1 >> 15)
    key = (65000 << 16) | 65001
    h = (key * 0x9E3779B1) & 0xFFFFFFFF
    assert int(pix_hash(np.array([key]))[0]) == h ^ (h >> 15)
    s = sel_of(np.array([key, (1 << 16) | 2, NONE, 5]), np.array([7, 3, 9, 0], np.uint64), [1, 2, 2], 3)
    # ids past len16 have length 0 here; (1, 2): 2 + 2 > 3 is filtered; empty; count 0
    assert s.tolist() == [(7 << 17) | (0x1FFFF - 130001), 0, 0, 0]
    assert sel_of(np.array([(1 << 16) | 2]), np.array([3], np.uint64), [1, 2, 2], 0).tolist() == [(3 << 17) | (0x1FFFF - 3)]


def test_view_refuses_null_arguments():
    import ctypes
    L = pkg.lib()
    info = (ctypes.c_int64 * pkg.PIX_INFO_WORDS)()
    assert L.bpe_debug_pix(None, info, None) == pkg.ERR_ARG
    assert L.bpe_debug_pix_shard(None, 0, info, None) == pkg.ERR_ARG
    assert L.bpe_debug_pix_hook(None, pkg.PIX_HOOK(0), None, 1) == pkg.ERR_ARG


# ---- the GPU driver ----------------------------------------------------------------------------------
class Watch:
    """A single context in the incremental mode and the oracle side by side.  The hook reads the
    live index at every call (where 0: before a batch, 1: after one), brings the oracle to the
    index's next_id and runs check_index; what it finds goes to `errors` (an exception raised in a
    ctypes callback is dropped), and done() asserts on all of it."""

    def __init__(self, samples, len16, batch=0, engine=None, oracle=None):
        if oracle is None:
            ids, off = flat(samples)
            oracle = OracleState(ids, off, len16, len(len16))
        self.st = oracle
        self.e = engine if engine is not None else make_engine(samples, len16)
        self.e.set_mode('incremental')
        self.e.stats_enable(True)
        self.errors, self.points, self.want, self.got = [], [], [], []
        self.base = oracle.n_tokens
        self.ml = 0
        self.n_built = 0
        self.expect_build = True
        self.only = None               # check only these wheres
        self.t_check = 0.0
        self.e.pix_hook(self._hook, batch)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.e.pix_hook(None)
        self.e.close()

    def _hook(self, where):
        t0 = time.perf_counter()
        try:
            self._check(where)
        except BaseException as x:   # noqa: B036 (nothing may leave a ctypes callback)
            self.errors.append((where, len(self.points), '%s: %s' % (type(x).__name__, str(x)[:1500])))
        self.t_check += time.perf_counter() - t0

    def oracle_to(self, n_tokens):
        while self.st.n_tokens < n_tokens:
            m = self.st.find_next_merge(self.ml, 2)
            assert m is not None, 'the oracle has no merge %d' % len(self.want)
            self.st.apply_merge(m[0], m[1])
            self.want.append(m)

    def _check(self, where):
        v = self.e.pix_view()
        assert v is not None, 'a hook call found no index'
        rec = {k: v[k] for k in ('status', 'tie', 'err', 'cap', 'pool_cap', 'pool_top', 'used', 'next_id', 'n_done')}
        rec['where'] = where
        rec['checked'] = False
        self.points.append(rec)
        if v['status'] == pkg.PIX_HOST:
            # the batch handed an iteration to the stream in mid-merge: this index is discarded and
            # another one built (the hand-off test checks that one)
            self.expect_build = True
            return
        if where == 0 and self.expect_build:
            self.n_built = v['next_id']
            self.expect_build = False
        if self.only is not None and where not in self.only:
            return
        self.oracle_to(v['next_id'])
        check_index(v, self.st.ids[:self.st.off[-1]], self.st.off, self.st.len16, self.ml, n_built=self.n_built)
        rec['checked'] = True

    def merge_until(self, ml, n):
        self.ml = ml
        self.expect_build = True       # (a single context builds its index on entry)
        got = self.e.merge_until(ml, 2, n)
        self.got += got
        return got

    def done(self, planned, host=0):
        """The merges are the oracle's, every planned check point was reached and passed."""
        assert not self.errors, self.errors[:3]
        while len(self.want) < len(self.got):     # (merges the stream made after the last point)
            m = self.st.find_next_merge(self.ml, 2)
            assert m is not None
            self.st.apply_merge(m[0], m[1])
            self.want.append(m)
        assert self.got == self.want[:len(self.got)] and len(self.got) == len(self.want), (
            len(self.got), len(self.want), self.got[:3], self.want[:3])
        checked = sum(p['checked'] for p in self.points)
        s = self.e.stats()
        print('index-state: %d merges, %d points, %d checked (%.2f s), pix_merges %d, pix_host %d, builds %d' % (
            len(self.got), len(self.points), checked, self.t_check, s['pix_merges'], s['pix_host'], s['pix_builds']))
        assert checked >= planned, (checked, planned)
        # every merge was made on the index, but for those the stream takes: before the first build
        # (the heavy-merge prefix of pix_merge_until), and one for every batch that handed over
        # (a where-1 point with PIX_HOST)
        prefix = self.points[0]['next_id'] - self.base
        handed = sum(p['status'] == pkg.PIX_HOST for p in self.points)
        assert s['pix_merges'] == len(self.got) - prefix - handed, (s, prefix, handed)
        assert s['pix_host'] == handed, (s, handed)
        if host == 0:
            assert handed == 0, [p for p in self.points if p['status'] == pkg.PIX_HOST][:2]
        else:
            assert handed >= host, s
        return s


# One superblock, so that a check costs milliseconds.  (Not the 2^14 slots that would also be one:
# pix_commit hands a merge to the stream when twice its list and 64 more claims would pass 70 % of
# the table, and the first merges of the three-letter corpora have lists of 7000 entries.)
SMALL = {'BPE_PIX_TABLE_FLOOR': str(1 << 16)}


def set_env(monkeypatch, env):
    for k, v in env.items():
        monkeypatch.setenv(k, v)


def random_samples(seed, n_tokens, A, n_samples=5, run_bias=0.1, lo=0):
    rng = np.random.default_rng(seed)
    out = []
    for L in rng.multinomial(n_tokens, np.ones(n_samples) / n_samples):
        runs = max(1, int(L))
        toks = rng.integers(lo, lo + A, runs)
        lens = np.where(rng.random(runs) >= run_bias, 1, rng.integers(2, 12, runs))
        out.append(np.repeat(toks, lens)[:L].astype(np.int32))
    return out


# ---- after the build -----------------------------------------------------------------------------
def build_corpora():
    """name -> (samples, len16, ml): the corpora of the after-build checks."""
    out = {}
    for A in (3, 30, 256, 280, 2000):
        out['random_A%d' % A] = (random_samples(A, 30000, A, run_bias=0.15), [1] * A, 0)
    for n in (4095, 4096, 4097, 8193):
        # runs of every parity across the 4096-position build blocks: 'x' * k ending at, across and
        # starting at each block edge, for k = 2 .. 9
        rng = np.random.default_rng(n)
        s = rng.integers(1, 12, n).astype(np.int32)
        for k in range(2, 10):
            for edge in range(4096, n + 1, 4096):
                at = edge - k + (k * 3) % (k + 1)
                s[max(0, at):min(n, at + k)] = 0
        out['size_%d' % n] = ([s], [1] * 12, 0)
    out['one_sample'] = ([random_samples(5, 20000, 40, 1)[0]], [1] * 40, 0)
    rng = np.random.default_rng(6)
    out['one_token_samples'] = ([rng.integers(0, 9, 1).astype(np.int32) for _ in range(6000)] +
                                random_samples(7, 20000, 9, 3) +
                                [np.zeros(0, np.int32)] * 5 + [rng.integers(0, 9, 1).astype(np.int32) for _ in range(3000)],
                                [1] * 9, 0)
    out['max_length_3'] = (random_samples(8, 30000, 30, run_bias=0.2), [1, 2] * 15, 3)
    return out


BUILD_CORPORA = None


def build_corpus(name):
    global BUILD_CORPORA
    if BUILD_CORPORA is None:
        BUILD_CORPORA = build_corpora()
    return BUILD_CORPORA[name]


BUILD_NAMES = ['random_A3', 'random_A30', 'random_A256', 'random_A280', 'random_A2000', 'size_4095', 'size_4096',
               'size_4097', 'size_8193', 'one_sample', 'one_token_samples', 'max_length_3']


@gpu
@pytest.mark.parametrize('fill', ['two_level', 'pairs'])
@pytest.mark.parametrize('name', BUILD_NAMES)
def test_index_after_the_build(name, fill, monkeypatch):
    """The freshly built index (where 0), then one batch of 8 merges (where 1), in both fill
    forms of the build."""
    set_env(monkeypatch, SMALL)
    if fill == 'pairs':
        monkeypatch.setenv('BPE_PIX_FILL_PAIRS', '1')
    samples, len16, ml = build_corpus(name)
    with Watch(samples, len16, batch=8) as w:
        w.merge_until(ml, 8)
        assert w.points and w.points[0]['where'] == 0 and w.points[0]['next_id'] == len(len16), w.points[:1]
        w.done(2)


def set_fill(monkeypatch, fill):
    if fill == 'pairs':
        monkeypatch.setenv('BPE_PIX_FILL_PAIRS', '1')


FILLS = pytest.mark.parametrize('fill', ['two_level', 'pairs'])


@gpu
@FILLS
def test_index_after_the_build_default_table(fill, monkeypatch):
    """The default table floor: 2^20 slots, 16 superblocks."""
    set_fill(monkeypatch, fill)
    samples, len16, ml = build_corpus('random_A280')
    with Watch(samples, len16, batch=8) as w:
        w.merge_until(ml, 8)
        assert w.points[0]['cap'] == 1 << 20
        w.done(2)


@gpu
@FILLS
@pytest.mark.parametrize('which', ['runs', 'empties'])
def test_index_after_the_build_placed_corpora(which, fill, monkeypatch):
    """The placed corpora of test_digest_stream.py (sites at chunk and region edges, runs of 600
    and 601, partial and emptied chunks), after the build and after one batch."""
    from test_digest_stream import placed_empties_corpus, placed_runs_corpus
    set_fill(monkeypatch, fill)
    samples, len16 = placed_runs_corpus() if which == 'runs' else placed_empties_corpus()
    with Watch(samples, len16, batch=8) as w:
        got = w.merge_until(4 if which == 'runs' else 0, 8)
        assert len(got) == 8
        w.done(2)


def count_sweeps_data():
    """10 MiB of random bytes in which every 256th build block (4096 positions; the build gives
    workgroup w the blocks w, w + 256, ..) is 'ab' repeats and another every 256th runs of 'z' of
    every parity: one workgroup counts 20 480 (a, b) and as many (b, a), another 40 000 positions
    of (z, z), far past the 16-bit LDS counters' sweep at 0x4000, while no pair of the corpus
    counts more than 65 536, so that the index is built on this corpus as it stands.  (The 24 MiB
    corpus of test_incremental.py's test_index_build_count_sweeps cannot be looked at like this:
    its pairs count millions, the stream takes those merges before a single context builds its
    index, and they dissolve the runs; a shard hands them to the host.)"""
    rng = np.random.default_rng(78)
    data = rng.integers(0, 256, 10 << 20, dtype=np.uint8)
    for blk in range(7, (10 << 20) // 4096, 256):
        data[blk * 4096:(blk + 1) * 4096] = np.resize(np.frombuffer(b'ab', np.uint8), 4096)
    for blk in range(100, (10 << 20) // 4096, 256):
        at = blk * 4096
        while at < (blk + 1) * 4096:
            n = int(rng.integers(2, 400))
            data[at:at + n] = ord('z')
            data[at + n] = ord('y')
            at += n + 1
    return data


PB = 4096                   # positions per build block
PH_WG_MAX = 256             # workgroups of the build's hot passes: block b goes to workgroup b % G
PH_SWEEP = 0x4000           # a 16-bit LDS counter at this value is swept into the slab


@gpu
@FILLS
def test_index_after_the_build_count_sweeps(fill, monkeypatch):
    """Per-workgroup counts past the build's 16-bit LDS counters (k_pix_hot_count's sweeps into
    the slab, which size and place every hot pair's list and give its count): after the build and
    after one batch of two merges only."""
    set_fill(monkeypatch, fill)
    data = count_sweeps_data()
    # what the case rests on: one workgroup of the count pass meets (a, b) more often than a
    # counter holds before its sweep (byte j is slot j + j // 2^20: a separator ends every sample)
    at = np.nonzero((data[:-1] == ord('a')) & (data[1:] == ord('b')))[0]
    at = at[(at + 1) % (1 << 20) != 0]
    n_slots = len(data) + len(data) // (1 << 20)
    G = min(PH_WG_MAX, (n_slots + PB - 1) // PB)
    per_wg = np.bincount(((at + at // (1 << 20)) // PB) % G, minlength=G)
    assert per_wg.max() > PH_SWEEP, ('corpus: no workgroup sweeps its (a, b) counter', int(per_wg.max()))
    e = pkg.Engine(0)
    cmap, nt, _ = e.add_latin1(data, sample_bytes=1 << 20)
    ids = cmap[data]
    st = OracleState(ids, np.arange(0, len(data) + 1, 1 << 20, dtype=np.int64), [1] * nt, nt)
    keys, counts = pair_count_arrays(st.ids, st.off)
    assert counts.max() <= 1 << 16, 'corpus: the stream would take the first merges'
    ab = (int(cmap[ord('a')]) << 16) | int(cmap[ord('b')])
    assert counts[np.searchsorted(keys, ab)] >= 10 * 2048
    with Watch(None, None, batch=2, engine=e, oracle=st) as w:
        assert len(w.merge_until(0, 2)) == 2
        w.done(2)
        assert w.points[0]['where'] == 0 and w.points[0]['next_id'] == nt


# ---- after every merge ---------------------------------------------------------------------------
def runs_corpus():
    """Runs whose (x, x) merges win: odd and even lengths, a trailing x, runs of the new token
    ((c, c): 'xxxx' -> 'cc'), chains 'abab' (whose merge makes (c, c) too), at sample edges."""
    rng = np.random.default_rng(21)
    parts = []
    for _ in range(2500):
        kind = int(rng.integers(0, 5))
        x = int(rng.integers(0, 3))
        if kind == 0:
            parts.append([x] * int(rng.integers(2, 14)))
        elif kind == 1:
            parts.append([3, 4] * int(rng.integers(1, 6)))
        elif kind == 2:
            parts.append([x] * int(rng.integers(2, 9)) + [5])
        elif kind == 3:
            parts.append(rng.integers(0, 8, int(rng.integers(1, 5))).tolist())
        else:
            parts.append([6] + [x] * (2 * int(rng.integers(1, 5)) + 1))
    toks = np.concatenate([np.array(p, np.int32) for p in parts])
    cuts = np.sort(rng.choice(np.arange(1, toks.size), 6, replace=False))
    return [s.astype(np.int32) for s in np.split(toks, cuts)], [1] * 8


def ab_corpus(ml):
    """The corpus of test_incremental.py's test_max_length_new_pairs_stay_on_the_index."""
    rng = np.random.default_rng(5 + ml)
    samples = []
    for _ in range(20):
        n = int(rng.integers(500, 3000))
        s = np.resize(np.array([0, 1], np.int32), n)
        noise = rng.random(n) < 0.15
        s[noise] = rng.integers(2, 20, int(noise.sum()))
        samples.append(s)
    return samples, [1] * 20


@gpu
@pytest.mark.parametrize('case', ['random_A3', 'random_A30', 'runs', 'ab_ml3', 'ab_ml5'])
def test_index_after_every_merge(case, monkeypatch):
    """A batch size of 1: the index after every merge, and between a tie's scan and its commit."""
    set_env(monkeypatch, SMALL)
    ml, merges = 0, 100
    if case.startswith('random'):
        A = int(case[8:])
        samples, len16 = random_samples(30 + A, 25000, A, run_bias=0.1), [1] * A
    elif case == 'runs':
        samples, len16 = runs_corpus()
    else:
        ml = int(case[5:])
        samples, len16 = ab_corpus(ml)
        merges = 80
    with Watch(samples, len16, batch=1) as w:
        w.only = (1,)
        got = w.merge_until(ml, merges)
        assert len(got) == merges, len(got)
        w.done(merges)
        ties = sum(p['tie'] == pkg.PIX_TIE_DECIDED for p in w.points if p['checked'])
        print(case, 'decided ties at check points:', ties)
        if case.startswith('random'):
            assert ties >= 1, 'no check point between a tie scan and its commit'
        if case == 'runs':
            assert any(a == b for a, b, _ in got), 'no (x, x) merge'


@gpu
def test_index_to_the_end_of_min_weight(monkeypatch):
    """Until no pair counts min_weight (PIX_DONE), checked after every merge and at the end."""
    set_env(monkeypatch, SMALL)
    samples, len16 = random_samples(41, 3000, 6, n_samples=3, run_bias=0.2), [1] * 6
    with Watch(samples, len16, batch=1) as w:
        w.only = (1,)
        got = w.merge_until(0, 0)
        assert 80 <= len(got) <= 2000, len(got)
        w.done(len(got) + 1)
        assert w.points[-1]['status'] == pkg.PIX_DONE and w.points[-1]['checked']


@gpu
def test_index_at_the_top_of_the_id_range(monkeypatch):
    """Token ids from 55 000 on, the top of the id range (BPE_MAX_VOCAB is 55 296: a larger id is
    refused with the sample): the key packing u << 16 | v with both ids past 2^15 and the tie
    order 0x1FFFF - (u + v) where u + v is largest, after every merge until the vocabulary limit
    hands over to the stream, which reports it (BPE_ERR_VOCAB)."""
    set_env(monkeypatch, SMALL)
    lo, A = 55000, 200
    samples = random_samples(51, 20000, A, lo=lo)
    len16 = [1] * (lo + A)
    room = pkg.MAX_VOCAB - (lo + A)
    with Watch(samples, len16, batch=1) as w:
        w.only = (1,)
        with pytest.raises(pkg.BpeError) as err:
            w.merge_until(0, 0)
        assert err.value.code == pkg.ERR_VOCAB
        assert not w.errors, w.errors[:3]
        checked = [p for p in w.points if p['checked']]
        print('top of the id range: %d merges, %d checked' % (len(w.want), len(checked)))
        assert len(checked) == room and checked[-1]['next_id'] == pkg.MAX_VOCAB, (len(checked), room)
        assert len(w.want) == room and w.e.num_tokens() == pkg.MAX_VOCAB
        s = w.e.stats()
        assert s['pix_merges'] == room and s['pix_host'] == 0, s
        assert w.e.samples() == w.st.samples()


# ---- batch boundaries at the default floors ------------------------------------------------------
@gpu
@pytest.mark.parametrize('batch', [8, 256])
def test_index_at_batch_boundaries(batch):
    """600 merges on 300 000 tokens, the default table and pool: every batch boundary."""
    samples, len16 = random_samples(61, 300000, 200, n_samples=9, run_bias=0.1), [1] * 200
    with Watch(samples, len16, batch=batch) as w:
        w.only = (1,)
        got = w.merge_until(0, 600)
        assert len(got) == 600
        w.done(-(-600 // batch))       # every boundary: 75 of 8; 256, 256 and 88


# ---- growth --------------------------------------------------------------------------------------
def points_of_growth(w):
    """(before, after) for every two successive points between which the table's capacity changed:
    it doubled, the change was seen at a where-0 point that was checked, and no tie was pending."""
    grown = [(a, b) for a, b in zip(w.points, w.points[1:]) if b['cap'] != a['cap']]
    assert all(b['cap'] == 2 * a['cap'] and b['where'] == 0 and b['checked'] for a, b in grown), grown[:2]
    assert all(a['tie'] == pkg.PIX_TIE_NONE for a, b in grown), 'a rehash under a decided tie'
    return grown


@gpu
def test_index_after_growth(monkeypatch):
    """A table floor of 2^12 slots and a pool slack of 2^10 entries: within 300 merges the table is
    rehashed twice as large at least twice and the pool grows; the index is checked before every
    batch (where 0: right after pix_reserve) and after it."""
    monkeypatch.setenv('BPE_PIX_TABLE_FLOOR', str(1 << 12))
    monkeypatch.setenv('BPE_PIX_POOL_SLACK', str(1 << 10))
    samples, len16 = random_samples(119, 30000, 20, run_bias=0.05), [1] * 20
    with Watch(samples, len16, batch=1) as w:
        got = w.merge_until(0, 300)
        assert len(got) == 300
        w.done(600)
        caps = [p['cap'] for p in w.points]
        pools = [p['pool_cap'] for p in w.points]
        print('growth: capacities', sorted(set(caps)), 'pool', sorted(set(pools)))
        assert len(points_of_growth(w)) >= 2, sorted(set(caps))
        assert all(b >= a for a, b in zip(pools, pools[1:])) and len(set(pools)) >= 2, sorted(set(pools))


def tied_corpus(shift):
    """Ten groups of twelve pairs (a, b) with one sum a + b and one count per group (60, 58, ..):
    each group's pairs tie on the packed key, so every merge but a group's last follows a tie-scan
    iteration.  Every site stands between two of 16 filler tokens, so a merge makes about as many
    new pairs as its pair had neighbours and the table, built a quarter full, passes 45 % near the
    end.  shift: so many pairs above all groups, merged first without ties, each of which moves
    every later iteration by one."""
    rng = np.random.default_rng(97)
    sites = []
    for g in range(10):
        for i in range(12):
            sites += [(100 * g + i, 100 * g + 50 - i)] * (60 - 2 * g)
    for j in range(shift):
        sites += [(990 + 2 * j, 991 + 2 * j)] * (100 + j)
    toks = []
    for k in rng.permutation(len(sites)):
        toks += [sites[k][0], sites[k][1], 1000 + int(rng.integers(0, 16))]
    # (six pairs that count once: they move the fill, which the table passes 45 % by, so that with
    # shift 2 the merge that passes it is the middle one of its batch)
    toks += [980, 981, 982, 983, 984, 985]
    return [np.array(toks, np.int32)], [1] * 1016


@gpu
def test_no_rehash_while_a_decided_tie_is_pending(monkeypatch):
    """Batches of 3 iterations over a corpus where tie scans and merges alternate: a boundary
    falls between a tie's scan and its commit every other batch.  The decision names its pair by
    slot, so pix_reserve must leave the table alone there, however full, and rehash after the
    commit.  The merge that passes 45 % must be the middle iteration of its batch for that; the
    three shifts try the three places it can have, so one of the runs sees it, and every boundary
    of all three is checked."""
    monkeypatch.setenv('BPE_PIX_TABLE_FLOOR', str(1 << 12))
    held = []
    for shift in (0, 1, 2):
        samples, len16 = tied_corpus(shift)
        with Watch(samples, len16, batch=3) as w:
            got = w.merge_until(0, 120 + shift)
            assert len(got) == 120 + shift
            w.done(2 * (120 // 3))
            grown = points_of_growth(w)
            full = [p for p in w.points if p['where'] == 0 and p['tie'] == pkg.PIX_TIE_DECIDED and
                    p['used'] * 20 > p['cap'] * 9]
            print('tied corpus, shift %d: capacities %s, decided ties at boundaries %d, of them past 45 %%: %d' % (
                shift, sorted({p['cap'] for p in w.points}),
                sum(p['where'] == 0 and p['tie'] == pkg.PIX_TIE_DECIDED for p in w.points), len(full)))
            assert len(grown) >= 1, 'the table never grew'
            held.append(len(full))
    assert max(held) >= 1, 'no decided tie at a boundary that would otherwise rehash'


# ---- hand-off and rebuild ------------------------------------------------------------------------
@gpu
def test_index_after_a_hand_off(monkeypatch):
    """'x' * 70000 (test_incremental.py's test_runs_in_the_index): the run is past the walk bound,
    the (x, x) merge goes to the stream, and the index built after it is checked like any other."""
    set_env(monkeypatch, SMALL)
    sample = np.array([1] + [0] * 70000 + [2, 0, 0, 0, 1], np.int32)
    with Watch([sample], [1, 1, 1], batch=1) as w:
        got = w.merge_until(0, 0)
        s = w.done(4, host=1)
        # (done() required pix_merges == the merges made - one per hand-off, exactly)
        assert s['pix_builds'] == 1 + s['pix_host'] and s['pix_merges'] > 0, s
        handed = [i for i, p in enumerate(w.points) if p['status'] == pkg.PIX_HOST]
        assert handed and any(p['checked'] and p['where'] == 0 for p in w.points[handed[0] + 1:]), w.points
        assert len(got) >= 4


# ---- sharded -------------------------------------------------------------------------------------
def shard_of_samples(samples, k):
    """distribute() of bpe_multi.cpp: contiguous runs of samples of about equal token counts."""
    total = sum(len(s) for s in samples)
    acc, out = 0, []
    for s in samples:
        out.append(min(k - 1, (acc + len(s) // 2) * k // total) if total else 0)
        acc += len(s)
    return np.array(out)


class Shards:
    """A multi-device context in the incremental mode, the oracle over the whole corpus, and per
    shard its own slice of the oracle's samples.  check(): every shard's index through the
    per-shard view, before anything reads the corpus (which would drop the indices).

    Between batches a shard's counts are those of the corpus ONE MERGE EARLIER with the merged
    pair at 0 whenever the view says delta_pending (pix_rank_end keeps the last merge's delta rows
    for the next batch's first all-reduce; k_pix_sites zeroed the pair at once), else those of the
    current corpus; lists and links are the current corpus's either way.  The oracle's counts are
    kept one merge behind for the first case; which case holds is read from the view."""

    def __init__(self, samples, len16, k):
        self.k = k
        self.samples = samples
        self.owner = shard_of_samples(samples, k)
        ids, off = flat(samples)
        self.st = OracleState(ids, off, len16, len(len16))
        self.e = pkg.Engine(devices=[0] * k, reduce='host')
        for i, l in enumerate(len16):
            self.e.set_token_len16(i, l)
        for s in samples:
            self.e.add_sample(s)
        self.e.set_mode('incremental')
        self.e.stats_enable(True)
        self.want, self.got = [], []
        self.prev_counts = None
        self.last = None
        self.checked = 0
        self.pending_seen = 0
        self.n_built = len(len16)

    def close(self):
        self.e.close()

    def call(self, ml, n):
        got = self.e.merge_until(ml, 2, n)
        for _ in got:
            self.prev_counts = pair_count_arrays(self.st.ids[:self.st.off[-1]], self.st.off)
            m = self.st.find_next_merge(ml, 2)
            assert m is not None
            self.st.apply_merge(m[0], m[1])
            self.want.append(m)
            self.last = m
        self.got += got
        assert self.got == self.want, (len(self.got), self.got[-3:], self.want[-3:])
        return got

    def check(self, ml):
        now = pair_count_arrays(self.st.ids[:self.st.off[-1]], self.st.off)
        for r in range(self.k):
            v = self.e.pix_view(shard=r)
            assert v is not None, ('shard %d holds no index after %d merges' % (r, len(self.got)), ml,
                                   {q: w for q, w in self.e.stats().items() if q.startswith('pix') or q == 'loop_host'})
            assert v['sharded'] == 1
            mine = np.nonzero(self.owner == r)[0]
            parts = [self.st.ids[self.st.off[i]:self.st.off[i + 1]] for i in mine]
            ids, off = flat(parts) if parts else (np.zeros(0, np.int32), np.zeros(1, np.int64))
            if v['delta_pending']:
                assert v['merged'] == 1 and self.last is not None
                keys, cnt = self.prev_counts
                cnt = cnt.copy()
                cnt[keys == ((self.last[0] << 16) | self.last[1])] = 0
                counts = (keys, cnt)
                self.pending_seen += 1
            else:
                counts = now
            try:
                check_index(v, ids, off, self.st.len16, ml, counts=counts, n_built=self.n_built)
            except AssertionError as x:
                raise AssertionError('shard %d of %d after %d merges: %s' % (r, self.k, len(self.got), x))
            self.checked += 1


def sharded_corpus():
    return random_samples(81, 30000, 40, n_samples=12, run_bias=0.1), [1, 1, 2, 1] * 10


@gpu
@pytest.mark.parametrize('dense', [False, True])
@pytest.mark.parametrize('k', [1, 2, 3])
def test_index_of_every_shard(k, dense, monkeypatch):
    """300 merges in calls of 7, both exchange layouts (BPE_XCHG_DENSE as in
    test_incremental_exchange_lanes_vs_dense_rows): every shard's index after every call."""
    set_env(monkeypatch, SMALL)
    if dense:
        monkeypatch.setenv('BPE_XCHG_DENSE', '1')
    samples, len16 = sharded_corpus()
    sh = Shards(samples, len16, k)
    try:
        calls = 0
        while len(sh.got) < 300:
            assert len(sh.call(0, 7)) == 7
            sh.check(0)
            calls += 1
        s = sh.e.stats()
        print('sharded k=%d dense=%s: %d calls, %d shard checks, %d with pending rows, stats %s' % (
            k, dense, calls, sh.checked, sh.pending_seen, {q: s[q] for q in ('pix_merges', 'pix_host', 'pix_builds')}))
        assert sh.checked == calls * k and calls >= 43
        assert sh.pending_seen > 0, 'no check point with pending delta rows'
        assert s['pix_host'] == 0 and s['pix_builds'] == k, s
        # (every shard makes every merge on its index, and the statistics sum over the shards)
        assert s['pix_merges'] == k * len(sh.got), (s['pix_merges'], k, len(sh.got))
        assert sh.e.samples() == sh.st.samples()
    finally:
        sh.close()


@gpu
def test_index_of_every_shard_max_length_changes_and_a_read(monkeypatch):
    """max_length changing between the calls (pix_rank_begin recomputes every maximum under the
    new filter), and midway a read of the samples, which drops the indices: the next call builds
    them again from the merged corpus, and the checks go on."""
    set_env(monkeypatch, SMALL)
    samples, len16 = sharded_corpus()
    sh = Shards(samples, len16, 3)
    try:
        plan = [0, 4, 6, 0, 3, 5] * 5
        drops = 0
        for i, ml in enumerate(plan):
            n = len(sh.call(ml, 7))
            if n == 7:
                sh.check(ml)
            else:
                # no pair left under this max_length: the batch ended, and the shards left the
                # global state (pix_rank_end); the next call builds the indices again
                assert all(sh.e.pix_view(shard=r) is None for r in range(3)), 'an index outlived its batch\'s end'
                sh.n_built = sh.st.n_tokens
                drops += 1
            if i == len(plan) // 2:
                assert sh.e.samples() == sh.st.samples()
                assert sh.e.pix_view(shard=0) is None, 'the read left the index alive'
                sh.n_built = sh.st.n_tokens
                drops += n == 7
        s = sh.e.stats()
        print('sharded max_length plan: %d merges, %d shard checks, %d pending, %d drops, stats %s' % (
            len(sh.got), sh.checked, sh.pending_seen, drops, {q: s[q] for q in ('pix_merges', 'pix_host', 'pix_builds')}))
        # (the ten calls without a max_length always find their seven merges)
        assert len(sh.got) >= 70 and sh.checked >= 3 * 10
        assert s['pix_host'] == 0 and s['pix_builds'] == 3 * (1 + drops), (s, drops)
        # (after the read too: every merge on every shard's index, none on the streaming rank loop)
        assert s['pix_merges'] == 3 * len(sh.got), (s['pix_merges'], len(sh.got))
    finally:
        sh.close()


@gpu
def test_view_refusals_on_the_device():
    """No index outside merge_until in a single context; BPE_ERR_ARG for the wrong kind of
    context, a bad shard, a bad batch and a stale sizing."""
    import ctypes
    e = make_engine([np.array([1, 2, 1, 2, 1, 2, 3], np.int32)], [1] * 4)
    try:
        e.set_mode('incremental')
        assert e.pix_view() is None
        assert e.merge_until(0, 2, 1) == [(1, 2, 3)]
        assert e.pix_view() is None
        L = pkg.lib()
        info = (ctypes.c_int64 * pkg.PIX_INFO_WORDS)()
        ptrs = (ctypes.c_void_p * len(pkg.PIX_ARRAYS))()
        assert L.bpe_debug_pix(e._ctx, None, None) == pkg.ERR_ARG
        assert L.bpe_debug_pix(e._ctx, info, ptrs) == pkg.ERR_ARG          # nothing to copy
        assert L.bpe_debug_pix_shard(e._ctx, 0, info, None) == pkg.ERR_ARG  # not a multi-device context
        assert L.bpe_debug_pix_hook(e._ctx, pkg.PIX_HOOK(0), None, 257) == pkg.ERR_ARG
        assert L.bpe_debug_pix_hook(e._ctx, pkg.PIX_HOOK(0), None, -1) == pkg.ERR_ARG
    finally:
        e.close()
    m = pkg.Engine(devices=[0, 0], reduce='host')
    try:
        with pytest.raises(pkg.BpeError) as err:
            m.pix_view()
        assert err.value.code == pkg.ERR_ARG
        with pytest.raises(pkg.BpeError) as err:
            m.pix_view(shard=2)
        assert err.value.code == pkg.ERR_ARG
        with pytest.raises(pkg.BpeError) as err:
            m.pix_hook(lambda where: None, 1)
        assert err.value.code == pkg.ERR_ARG
        assert m.pix_view(shard=1) is None
    finally:
        m.close()
