"""The maintained state of the streaming engine: once pairs of merged tokens win, every pair with
an id >= 256 (a cold pair) is kept in an exact hash table and the 65 536 hot bins are kept exact
too; a merge pass (MODE_INCR) recounts only the pairs with a side in {a, b, c}.  Every GPU test
here drives the merge loop in batches against the oracle and requires, after every batch (in the
'host' mode after every merge), the oracle's merges, the oracle's corpus and, wherever the engine
reports the maintained state, tables equal to a recount of that corpus by pair_counts() below: all
hot bins, every cold pair, no key twice.  Every test also requires that the state was reached.
The corpora place sites at the limits of this pass: chunk, region and sample edges, runs, the four
LDS rows and their limit (INCR_RLIM), the LDS hash and its overflow, row counters past 16 bits, the
cold table's block maxima, its rebuild, and the end of the vocabulary."""
import numpy as np
import pytest

from bpe_amd import make_engine, pkg
from oracle import OracleState
from test_digest_stream import flat, placed_empties_corpus, placed_runs_corpus

gpu = pytest.mark.gpu

HOT = 256                   # ids below it are hot; a pair with an id >= HOT is cold
EMPTY = 0xFFFFFFFF          # a hole of the cold table's dense view
INCR_RLIM = 18432           # counters per LDS row of the MODE_INCR pass (bpe_pass.hip.h)
SEL_FULL_EVERY = 16         # every such selection of a batch scans the whole cold table
BATCHES = [8, 40]           # 8: a full selection and seven from the block maxima; 40: full scans
                            # inside a batch (40 > SEL_FULL_EVERY)
MODES = ['loop', 'host']


# ---- 2. the reference counter --------------------------------------------------------------------
def pair_count_arrays(ids, off):
    """(keys, counts): every adjacent pair inside a sample as a << 16 | b (sorted, unique) and its
    count.  A pair (x, x) counts only at even offsets from the start of its run of equal tokens
    within the sample (leftmost non-overlapping, core.ts:285-290).  No max_length filter: the
    tables hold every pair."""
    ids = np.asarray(ids, np.int64)
    off = np.asarray(off, np.int64)
    n = ids.size
    if n < 2:
        return np.zeros(0, np.int64), np.zeros(0, np.int64)
    x, y = ids[:-1], ids[1:]
    valid = np.ones(n - 1, bool)
    cut = off[1:-1]
    cut = cut[(cut > 0) & (cut < n)]
    valid[cut - 1] = False                      # the pair across a sample boundary
    idx = np.arange(n, dtype=np.int64)
    start = np.ones(n, bool)
    start[1:] = y != x
    first = off[:-1]
    start[first[first < n]] = True              # a run ends with its sample
    run_start = np.maximum.accumulate(np.where(start, idx, 0))
    odd = ((idx[:-1] - run_start[:-1]) & 1) == 1
    valid &= ~((x == y) & odd)
    x, y = x[valid], y[valid]
    present = np.zeros(1 << 16, bool)
    present[ids] = True
    toks = np.nonzero(present)[0]
    V = toks.size
    if V * V <= 1 << 22:
        # few distinct tokens: a dense count over their ranks (no sort of the pairs)
        rank = np.cumsum(present) - 1
        c = np.bincount(rank[x] * V + rank[y], minlength=V * V)
        nz = np.nonzero(c)[0]
        keys = (toks[nz // V] << 16) | toks[nz % V]
        order = np.argsort(keys, kind='stable')
        return keys[order], c[nz][order].astype(np.int64)
    keys, counts = np.unique((x << 16) | y, return_counts=True)
    return keys, counts.astype(np.int64)


def pair_counts(ids, off):
    """{a << 16 | b: count} of pair_count_arrays."""
    keys, counts = pair_count_arrays(ids, off)
    return dict(zip(keys.tolist(), counts.tolist()))


def test_pair_counts_matches_the_oracles_counter():
    """The numpy counter against OracleState.count_pairs(None) on 40 seeded run-heavy corpora
    (alphabets 2 to 20, 1 to 9 samples, empty samples included).  The oracle's counter allocates
    V * V entries, so it cannot serve the large vocabularies below; this one can."""
    for seed in range(40):
        rng = np.random.default_rng(seed)
        A = int(rng.integers(2, 21))
        samples = []
        for _ in range(int(rng.integers(1, 10))):
            if rng.random() < 0.2:
                samples.append(np.zeros(0, np.int32))
                continue
            runs = int(rng.integers(1, 120))
            toks = rng.integers(0, A, size=runs)
            lens = np.where(rng.random(runs) < 0.5, 1, rng.integers(2, 12, size=runs))
            samples.append(np.repeat(toks, lens).astype(np.int32))
        if not any(len(s) for s in samples):
            samples.append(np.array([0, 0, 0, 1], np.int32))
        ids, off = flat(samples)
        st = OracleState(ids, off, [1] * A, A)
        pa, pb, pc, _ = st.count_pairs(None)
        want = {(int(a) << 16) | int(b): int(c) for a, b, c in zip(pa, pb, pc)}
        assert pair_counts(ids, off) == want, seed


def check_maintained(e, st):
    """The engine's maintained tables against a recount of the oracle's corpus."""
    assert e.is_maintained()
    keys, counts = pair_count_arrays(st.ids[:st.off[-1]], st.off)
    a, b = keys >> 16, keys & 0xFFFF
    is_hot = (a < HOT) & (b < HOT)
    want_hot = np.zeros(pkg.HOT_BINS, np.int64)
    want_hot[b[is_hot] * 256 + a[is_hot]] = counts[is_hot]
    hot, ck, cc = e.maintained_tables()
    hot = hot.astype(np.int64)
    bad = np.nonzero(hot != want_hot)[0]
    assert bad.size == 0, ('hot bins (a, b, kept, want)',
                           [(int(i) & 255, int(i) >> 8, int(hot[i]), int(want_hot[i])) for i in bad[:8]])
    # no key twice among the claims (dead claims, with count 0, included)
    claimed = ck[ck != EMPTY]
    uniq, n_of = np.unique(claimed, return_counts=True)
    assert uniq.size == claimed.size, ('keys claimed twice (a, b, times)',
                                       [(int(k) >> 16, int(k) & 0xFFFF, int(m))
                                        for k, m in zip(uniq[n_of > 1][:8], n_of[n_of > 1][:8])])
    live = (ck != EMPTY) & (cc > 0)
    order = np.argsort(ck[live], kind='stable')
    got_k, got_c = ck[live][order].astype(np.int64), cc[live][order].astype(np.int64)
    want_k, want_c = keys[~is_hot], counts[~is_hot]
    if not (np.array_equal(got_k, want_k) and np.array_equal(got_c, want_c)):
        got = dict(zip(got_k.tolist(), got_c.tolist()))
        want = dict(zip(want_k.tolist(), want_c.tolist()))
        diff = [(k >> 16, k & 0xFFFF, got.get(k, 0), want.get(k, 0))
                for k in sorted(set(got) | set(want)) if got.get(k, 0) != want.get(k, 0)]
        raise AssertionError(('cold pairs (a, b, kept, want): %d differ' % len(diff), diff[:8]))


# ---- 1. the accessor's refusals ------------------------------------------------------------------
def test_accessor_refuses_null_arguments():
    import ctypes
    L = pkg.lib()
    m, n = ctypes.c_int(7), ctypes.c_int64(7)
    hot = np.zeros(pkg.HOT_BINS, np.uint64)
    assert L.bpe_table_state(None, ctypes.byref(m)) == pkg.ERR_ARG
    assert L.bpe_debug_tables(None, hot.ctypes.data, None, None, 0, ctypes.byref(n)) == pkg.ERR_ARG
    assert (m.value, n.value) == (7, 7)


@gpu
def test_accessor_refuses_a_multi_device_context_and_null_outputs():
    import ctypes
    e = pkg.Engine(devices=[0, 0], reduce='host')
    try:
        for call in (e.is_maintained, e.maintained_tables):
            with pytest.raises(pkg.BpeError) as err:
                call()
            assert err.value.code == pkg.ERR_ARG
    finally:
        e.close()
    e = make_engine([np.array([HOT, HOT + 1] * 8, np.int32)], [1] * (HOT + 2))
    try:
        L = pkg.lib()
        n = ctypes.c_int64()
        hot = np.zeros(pkg.HOT_BINS, np.uint64)
        assert L.bpe_table_state(e._ctx, None) == pkg.ERR_ARG
        assert L.bpe_debug_tables(e._ctx, None, None, None, 0, ctypes.byref(n)) == pkg.ERR_ARG
        assert L.bpe_debug_tables(e._ctx, hot.ctypes.data, None, None, 0, None) == pkg.ERR_ARG
        assert L.bpe_debug_tables(e._ctx, hot.ctypes.data, None, None, 4, ctypes.byref(n)) == pkg.ERR_ARG
        # a fresh context is not in the state, and has no cold table yet
        assert not e.is_maintained()
        assert e.maintained_tables()[1].size == 0
    finally:
        e.close()


# ---- 3. the driver -------------------------------------------------------------------------------
class Run:
    """An engine and the oracle side by side.  batch(): merges on both; check(): the corpus, and
    the tables wherever the engine is in the maintained state (`maintained` counts those checks,
    `checks` all of them)."""

    def __init__(self, samples, len16, extra=1024):
        ids, off = flat(samples)
        self.st = OracleState(ids, off, len16, len(len16), extra=extra)
        self.e = make_engine(samples, len16)
        self.e.stats_enable(True)
        self.merges = []
        self.maintained = self.checks = 0
        self.in_state = []          # per check: whether the engine was in the maintained state

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.e.close()

    def check(self):
        ids, off = self.e.read_corpus()
        assert off.tolist() == self.st.off.tolist()
        assert np.array_equal(ids, self.st.ids[:self.st.off[-1]])
        self.checks += 1
        m = self.e.is_maintained()
        self.in_state.append(m)
        if m:
            check_maintained(self.e, self.st)
            self.maintained += 1

    def batch(self, max_length, n, mode):
        """n merges: 'loop' merge_until and one check; 'host' find_next_merge / apply_merge one at
        a time, the check after every merge.  Returns how many merges there were."""
        if mode == 'loop':
            w = self.st.merge_until(max_length, 2, n)
            got = self.e.merge_until(max_length, 2, n)
            assert got == w
            self.merges += w
            self.check()
            return len(w)
        for i in range(n):
            w = self.st.merge_until(max_length, 2, 1)
            m = self.e.find_next_merge(max_length, 2)
            if not w:
                assert m is None
                return i
            assert [m] == w
            assert self.e.apply_merge(m[0], m[1], self.e.num_tokens()) == m[2]
            self.merges += w
            self.check()
        return n

    def run(self, plan, mode):
        """plan: (max_length, merges) per batch."""
        for max_length, n in plan:
            self.batch(max_length, n, mode)
        return self


def cold(len16):
    """len16 of a corpus whose ids were moved up by HOT: 256 unused entries, then the values."""
    return [1] * HOT + list(len16)


def separated(rng, sites, fill, gap=1):
    """The sites (token lists) in random order, `gap` random tokens of `fill` after each."""
    out = []
    for i in rng.permutation(len(sites)):
        out.extend(sites[i])
        out.extend(rng.choice(fill, size=gap).tolist())
    return np.array(out, np.int32)


# ---- a. random, all cold -------------------------------------------------------------------------
RANDOM = [  # tokens, base ids, run bias, samples, merges
    (6000, 3, 0.3, 1, 60), (9000, 7, 0.05, 7, 90), (40000, 20, 0.0, 3, 150),
    (120000, 60, 0.3, 17, 100), (300000, 12, 0.7, 200, 80), (300000, 40, 0.05, 5, 120),
]


def random_cold_corpus(seed, lo=HOT):
    """Seeded corpus over ids lo .. with runs as in test_gpu_parity's random_corpus (a run of 2 to
    12, one in ten of up to 900, with probability run_bias), len16 in {1, 2}."""
    n, A, bias, n_samples, merges = RANDOM[seed]
    rng = np.random.default_rng(1000 + seed)
    samples = []
    per = max(1, n // n_samples)
    for _ in range(n_samples):
        L = int(rng.integers(0, 2 * per + 1))
        runs = max(1, L)
        toks = rng.integers(lo, lo + A, size=runs)
        lens = np.where(rng.random(runs) >= bias, 1,
                        np.where(rng.random(runs) < 0.9, rng.integers(2, 13, size=runs),
                                 rng.integers(2, 901, size=runs)))
        samples.append(np.repeat(toks, lens)[:L].astype(np.int32))
    len16 = [1] * lo + [int(v) for v in rng.integers(1, 3, size=A)]
    return samples, len16, merges, rng


def random_plan(rng, merges, bs):
    """Batches of bs with max_length drawn from {0, 4, 6} per batch (the block maxima are computed
    under a max_length: a batch's first selection must recompute them).  A batch under a
    max_length may run out of pairs; the plan has as many batches again at 0 behind it."""
    k = (merges + bs - 1) // bs
    return [(int(rng.choice([0, 4, 6])), bs) for _ in range(k)] + [(0, bs)] * k


def run_random(seed, mode, bs, lo=HOT):
    samples, len16, merges, rng = random_cold_corpus(seed, lo)
    with Run(samples, len16) as r:
        for max_length, n in random_plan(rng, merges, bs):
            if len(r.merges) >= merges:
                break
            r.batch(max_length, n, mode)
        print(seed, mode, bs, len(r.merges), r.maintained, r.checks, r.e.stats())
        assert len(r.merges) >= min(merges, 40), len(r.merges)
        # entered with the third merge, and kept
        assert r.maintained >= r.checks - (1 if mode == 'loop' else 2), (r.maintained, r.checks, r.in_state)
        assert r.maintained >= 2


@gpu
@pytest.mark.parametrize('bs', BATCHES)
@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('seed', range(len(RANDOM)))
def test_random_all_cold(seed, mode, bs):
    run_random(seed, mode, bs)


# ---- b. mixed hot and cold -----------------------------------------------------------------------
def mixed_corpus():
    """300 k tokens over the ids 200 .. 330: a merge pair, its neighbours and the new token fall on
    both sides of 256 (k_incr_invalidate's rows and columns, the hot / cold split of the adds)."""
    rng = np.random.default_rng(77)
    samples = [rng.integers(200, 331, size=n).astype(np.int32) for n in (150_000, 0, 100_000, 50_000)]
    return samples, [1] * 331


@gpu
@pytest.mark.parametrize('bs', BATCHES)
@pytest.mark.parametrize('mode', MODES)
def test_mixed_hot_and_cold(mode, bs):
    samples, len16 = mixed_corpus()
    with Run(samples, len16) as r:
        total = 80 if mode == 'loop' else 40
        r.run([(0, bs)] * (total // bs), mode)
        print(r.maintained, r.checks, r.in_state, r.e.stats())
        ab = np.array([m[:2] for m in r.merges])
        assert (ab < HOT).any() and (ab >= HOT).any(), 'corpus: merges on one side of 256 only'
        assert r.maintained >= r.checks // 2 and r.maintained >= 2, (r.maintained, r.checks, r.in_state)


# ---- c. edges of the stream ----------------------------------------------------------------------
def entry_sample(rng, ids4, counts=(700, 650)):
    """A sample whose two planted pairs merge first (the two host iterations that enter the
    maintained state), so that everything after them is recounted by the MODE_INCR pass."""
    p, q, r, s = ids4
    sites = [[p, q]] * counts[0] + [[r, s]] * counts[1]
    return separated(rng, sites, np.arange(HOT + 100, HOT + 190))


def cold_runs_corpus():
    samples, len16 = placed_runs_corpus()
    samples = [s + HOT for s in samples]
    len16 = cold(len16) + [1] * 4
    V = len(len16)
    samples.append(entry_sample(np.random.default_rng(5), (V - 4, V - 3, V - 2, V - 1)))
    return samples, len16


def cold_empties_corpus():
    samples, len16 = placed_empties_corpus()
    return [s + HOT for s in samples], cold(len16)


def xx_runs_corpus():
    """An X X merge of a cold token with runs of every length 2 to 9 and of 1023, 1024 and 70 001
    (273 chunks: across regions and workgroups), each run between two other tokens and one at a
    sample's end and start.  len16[X] = 3 and max_length 4 keep (X, X) out of the first batch (in
    which the state is entered); the second, at 0, begins with it, and then merges its runs again
    and again."""
    rng = np.random.default_rng(9)
    X = HOT + 50
    fill = np.arange(HOT, HOT + 40)
    parts = [rng.choice(fill, size=3000)]
    for L in list(range(2, 10)) + [1023, 1024, 70_001, 5, 8]:
        parts += [np.full(L, X), rng.choice(fill, size=int(rng.integers(1, 700)))]
    s0 = np.concatenate(parts).astype(np.int32)
    s1 = np.concatenate([np.full(7, X), rng.choice(fill, size=2000), np.full(6, X)]).astype(np.int32)
    s2 = np.concatenate([np.full(4, X), rng.choice(fill, size=50_000)]).astype(np.int32)
    len16 = [1] * (HOT + 51)
    len16[X] = 3
    return [s0, s1, s2], len16, X


def run_placed_runs(mode):
    samples, len16 = cold_runs_corpus()
    V = len(len16)
    with Run(samples, len16) as r:
        r.run([(4, 8), (4, 8)] if mode == 'loop' else [(4, 9)], mode)
        print(r.merges, r.in_state, r.e.stats())
        assert [m[:2] for m in r.merges[:2]] == [(V - 4, V - 3), (V - 2, V - 1)], r.merges[:2]
        assert r.merges[2:7] == [(HOT + 0, HOT + 1, 526), (HOT + 7, HOT + 8, 325), (HOT + 2, HOT + 3, 270),
                                 (HOT + 4, HOT + 5, 200), (HOT + 10, HOT + 11, 171)], r.merges[2:7]
        assert r.maintained == (r.checks if mode == 'loop' else r.checks - 1), r.in_state


@gpu
@pytest.mark.parametrize('mode', MODES)
def test_placed_runs_chains_and_boundaries_maintained(mode):
    run_placed_runs(mode)


def run_placed_empties(mode):
    samples, len16 = cold_empties_corpus()
    with Run(samples, len16) as r:
        r.run([(0, 8)] * 3 if mode == 'loop' else [(0, 17)], mode)
        print(r.merges, r.in_state, r.e.stats())
        tail = [m for m in r.merges if m[2] == 130]
        assert len(tail) == 3 and tail[0][0] == HOT + 14 and tail[1][1] == HOT + 15, r.merges
        assert tail[2][:2] == (len(len16) + r.merges.index(tail[0]), len(len16) + r.merges.index(tail[1]))
        assert r.merges[16] == (len(len16) + r.merges.index(tail[2]), HOT + 9, 100), r.merges[16]
        assert r.maintained == (r.checks if mode == 'loop' else r.checks - 1), r.in_state


@gpu
@pytest.mark.parametrize('mode', MODES)
def test_placed_sites_beyond_emptied_chunks_maintained(mode):
    run_placed_empties(mode)


def run_xx_runs(mode):
    samples, len16, X = xx_runs_corpus()
    with Run(samples, len16) as r:
        r.run([(4, 8), (0, 8), (0, 8)] if mode == 'loop' else [(4, 8), (0, 10)], mode)
        print(r.merges, r.in_state, r.e.stats())
        assert all(X not in m[:2] for m in r.merges[:8]), r.merges[:8]
        assert r.merges[8][:2] == (X, X) and r.merges[8][2] > 35_000, r.merges[8]
        c = len(len16) + 8
        assert (c, c) in [m[:2] for m in r.merges[9:]], r.merges[9:]
        assert r.maintained == (r.checks if mode == 'loop' else r.checks - 1), r.in_state


@gpu
@pytest.mark.parametrize('mode', MODES)
def test_cold_xx_runs_of_every_length(mode):
    run_xx_runs(mode)


# ---- d. pairs among a, b and c -------------------------------------------------------------------
def pattern_corpus(V):
    """Short patterns over the highest ids below V, each repeated so that its pair (a, b) is the
    winner in turn, after two planted pairs that enter the state.  With the merge (a, b) -> c:
        a a b          -> (a, c)          [b < a: (a, b) goes before (a, a) at equal W]
        a b b          -> (c, b)          [a < b]
        a b a b        -> (c, c)
        b a b a, a b   -> (b, c), (c, a)
        a a a a a      -> (c, c), (c, a)  [the merge (a, a)]
    Each of these pairs lands in exactly one of the pass's four rows or its hash, once.  V (the
    first new id) odd and even: the rows' used part is rounded to a dword."""
    rng = np.random.default_rng(V)
    t = iter(range(V - 1, V - 41, -1))
    fill = np.arange(HOT, HOT + 24)
    sites = []
    planted = []

    def plant(pattern, n, pair):
        sites.extend([pattern] * n)
        planted.append(pair)

    p, q, r, s = next(t), next(t), next(t), next(t)
    plant([p, q], 500, (p, q))
    plant([r, s], 460, (r, s))
    a, b = next(t), next(t)             # a > b
    plant([a, a, b], 400, (a, b))
    b, a = next(t), next(t)             # a < b
    plant([a, b, b], 360, (a, b))
    a, b = next(t), next(t)
    plant([a, b, a, b], 160, (a, b))
    a, b = next(t), next(t)
    plant([b, a, b, a], 100, (a, b))
    sites.extend([[a, b]] * 180)
    a = next(t)
    plant([a] * 5, 120, (a, a))
    return [separated(rng, sites, fill)], [1] * V, planted


def run_patterns(V, mode):
    samples, len16, planted = pattern_corpus(V)
    with Run(samples, len16) as r:
        r.run([(0, 8)] * 3, mode)
        print(r.merges, r.in_state)
        got = [m[:2] for m in r.merges]
        assert got[:2] == planted[:2], got[:2]
        for pair in planted[2:]:
            assert pair in got[2:], (pair, got)
        assert r.maintained == (r.checks if mode == 'loop' else r.checks - 1), r.in_state


@gpu
@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('V', [320, 321])
def test_pairs_among_a_b_and_c(V, mode):
    run_patterns(V, mode)


# ---- e. the rows' limit --------------------------------------------------------------------------
def rows_limit_corpus():
    """18 440 registered tokens.  The neighbours of a and b of the third merge include the ids
    18 430 .. 18 439, both sides of INCR_RLIM, as left and as right neighbours (y a y b y: all four
    rows); a later merge's own tokens lie past the limit; every other id >= 256 occurs as filler."""
    V = INCR_RLIM + 8
    rng = np.random.default_rng(18)
    a, b, p, q, r, s = 300, 301, 310, 311, 312, 313
    edge = list(range(INCR_RLIM - 2, INCR_RLIM + 8))
    used = {a, b, p, q, r, s, *edge}
    sites = [[p, q]] * 500 + [[r, s]] * 450 + [[a, b]] * 300
    for y in edge:
        sites += [[y, a, y, b, y]] * (3 + y % 4)
    u, v = INCR_RLIM + 3, INCR_RLIM + 4          # a merge of two tokens past the limit
    sites += [[u, v]] * 250
    for y in (INCR_RLIM - 1, INCR_RLIM, 320, 321):
        sites += [[y, u, v, y]] * 6
    fill = np.array([i for i in range(HOT, INCR_RLIM - 2) if i not in used])
    gaps = rng.permutation(fill)
    out = []
    order = rng.permutation(len(sites))
    assert len(gaps) >= len(order)
    for k, i in enumerate(order):
        out.extend(sites[i])
        out.append(int(gaps[k]))
    out.extend(gaps[len(order):].tolist())
    return [np.array(out, np.int32)], [1] * V, [(p, q), (r, s), (a, b), (u, v)]


@gpu
@pytest.mark.parametrize('mode', MODES)
def test_neighbours_on_both_sides_of_the_rows_limit(mode):
    samples, len16, planted = rows_limit_corpus()
    with Run(samples, len16) as r:
        r.run([(0, 8), (0, 8)] if mode == 'loop' else [(0, 10)], mode)
        print(r.merges, r.in_state)
        got = [m[:2] for m in r.merges]
        assert got[:3] == planted[:3] and planted[3] in got, got
        assert r.maintained == (r.checks if mode == 'loop' else r.checks - 1), r.in_state


@gpu
@pytest.mark.parametrize('mode', MODES)
def test_vocabulary_past_the_rows_limit(mode):
    """The patterns of (d) on a vocabulary that is past INCR_RLIM when the state begins: every
    pair of c, and every pair of a or b with a token past the limit, goes to the LDS hash."""
    run_patterns(INCR_RLIM + 8, mode)


# ---- f. the LDS hash's overflow ------------------------------------------------------------------
def hash_overflow_corpus():
    """a b y_i a b y_i+1 .. with 2000 distinct y_i, contiguous at the start of the corpus: after
    the merge one workgroup's 4096 slots hold more than 1300 sites, so more than 2600 distinct
    (c, y_i) and (y_i, c) for the 2048 slots of its hash (then 8 probes, then global adds)."""
    rng = np.random.default_rng(6)
    a, b = 300, 301
    ys = np.arange(400, 2400)
    block = np.empty(3 * len(ys), np.int64)
    block[0::3], block[1::3], block[2::3] = a, b, rng.permutation(ys)
    p, q, r, s = 310, 311, 312, 313
    rest = separated(rng, [[p, q]] * 2600 + [[r, s]] * 2300, ys)
    return [np.concatenate([block, rest]).astype(np.int32)], [1] * 2400, (a, b)


@gpu
@pytest.mark.parametrize('mode', MODES)
def test_lds_hash_overflows_to_global_adds(mode):
    samples, len16, ab = hash_overflow_corpus()
    assert sum(len(s) for s in samples) < 1_000_000      # one chunk per region
    with Run(samples, len16) as r:
        r.run([(0, 8)], mode)
        print(r.merges, r.in_state)
        assert r.merges[2] == ab + (2000,), r.merges[:3]
        assert r.maintained == (r.checks if mode == 'loop' else r.checks - 1), r.in_state


# ---- g. row counters past 16 bits ----------------------------------------------------------------
def wide_rows_corpus():
    """a y a y .. for 12 M tokens (12 chunks per region: a workgroup's 49 152 slots hold 24 576 of
    (a, y) and of (y, a), past the rows' 0x4000 screen), len16[y] = 9 so that max_length 8 keeps
    both pairs out of every selection; a cold random part with (p, q) and (r, s), which enter the
    state, and 2000 sites of (a, b), whose MODE_INCR pass recounts the 6 M."""
    rng = np.random.default_rng(16)
    a, y, b, p, q, r, s = 300, 301, 302, 310, 311, 312, 313
    big = np.empty(12_000_000, np.int32)
    big[0::2], big[1::2] = a, y
    fill = np.arange(320, 520)
    part = separated(rng, [[p, q]] * 3000 + [[r, s]] * 2500 + [[a, b]] * 2000, fill, gap=12)
    len16 = [1] * 520
    len16[y] = 9
    return [big, part], len16, (a, y, b)


@gpu
def test_row_counters_past_16_bits():
    """No selection can see a miscount of (a, y) or (y, a) under max_length 8; only the tables'
    check can.  The last batch, at 0, must bring the oracle's (a, y) first.  (12 M tokens is the
    limit this case is there for: it takes longer than the others.)"""
    samples, len16, (a, y, b) = wide_rows_corpus()
    with Run(samples, len16) as r:
        r.run([(8, 3), (8, 5), (0, 2)], 'loop')
        print(r.merges, r.in_state, r.e.stats())
        assert [m[:2] for m in r.merges[:3]] == [(310, 311), (312, 313), (a, b)], r.merges[:3]
        assert all(y not in m[:2] for m in r.merges[:8]), r.merges[:8]
        assert r.merges[8][:2] == (a, y) and r.merges[8][2] > 5_990_000, r.merges[8]
        assert r.maintained == r.checks == 3, r.in_state


# ---- h. block maxima -----------------------------------------------------------------------------
TIES = [(2, 270), (16, 262), (17, 254), (40, 246)]      # pairs in the group, their W


def block_maxima_corpus():
    """300 k tokens over 800 cold ids (some 250 000 distinct pairs: well over 100 blocks of 1024
    entries) and, on 200 ids of their own, planted winners (a_i, b_i) and (a_i, z_i) in descending
    counts (the merge of (a_i, b_i) zeroes the entry (a_i, z_i), the next best and so some block's
    maximum) and R3 ties of 2, 16, 17 and 40 pairs of equal W and equal a + b."""
    rng = np.random.default_rng(8)
    buf = rng.integers(HOT + 200, HOT + 1000, size=300_000).astype(np.int32)
    t = iter(range(HOT, HOT + 200))
    sites = []
    for i in range(6):
        a, b, z = next(t), next(t), next(t)
        sites += [(a, b)] * (400 - 20 * i) + [(a, z)] * (395 - 20 * i)
    for n, W in TIES:
        lo = [next(t) for _ in range(n)]
        hi = [next(t) for _ in range(n)]
        for k in range(n):
            sites += [(lo[k], hi[n - 1 - k])] * W
    cells = rng.permutation(len(buf) // 4 - 2)[:len(sites)] + 1
    for (x, y), c in zip(sites, cells):
        buf[4 * c + 1:4 * c + 3] = [x, y]
    return [buf[:200_000], buf[200_000:]], [1] * (HOT + 1000)


@gpu
def test_zeroed_block_maxima_keep_the_loop_on_the_device():
    """The twelve planted winners in one call.  Every merge zeroes its own pair's entry, which was
    the best of the table and so its block's maximum, and with it (a_i, z_i), the next best.
    Unless k_incr_invalidate flags those blocks, the next selection from the block maxima finds a
    maximum that no entry holds and hands the iteration to the host, which selects correctly: no
    table and no merge shows it.  The count of merges decided on the device does: all but the
    two that enter the state."""
    samples, len16 = block_maxima_corpus()
    with Run(samples, len16) as r:
        r.batch(0, 12, 'loop')
        stats = r.e.stats()
        print(r.merges, stats)
        assert [m[2] for m in r.merges] == [400 - 20 * (i // 2) - 5 * (i % 2) for i in range(12)], r.merges
        assert r.maintained == 1
        assert stats['loop_host'] == 1 and stats['incr_launches'] == 10, stats


@gpu
@pytest.mark.parametrize('mode,bs', [('loop', 8), ('loop', 40), ('host', 8)])
def test_block_maxima_and_ties(mode, bs):
    """The winners, then the tie groups in turn.  'loop' takes all four groups; 'host' (the check
    after every merge, select_from_table's maintained branch) the groups of 2, 16 and 17, so a
    tie of more than MAX_CAND pairs there too: the group of 40 only repeats that."""
    samples, len16 = block_maxima_corpus()
    groups = TIES if mode == 'loop' else TIES[:3]
    total = 12 + sum(n for n, _ in groups) + 5
    with Run(samples, len16) as r:
        for _ in range((total + bs - 1) // bs):
            r.batch(0, bs, mode)
        stats = r.e.stats()
        print(r.merges, r.in_state, stats)
        W = [m[2] for m in r.merges[:12]]
        assert W == sorted(W, reverse=True) and W[0] == 400 and W[11] == 295, r.merges[:12]
        at = 12
        for n, w in groups:
            assert all(m[2] == w for m in r.merges[at:at + n]), (n, w, r.merges[at:at + n])
            at += n
        assert len(r.merges) >= at
        assert r.maintained >= r.checks - (1 if mode == 'loop' else 2), r.in_state
        if mode == 'loop':
            # entering the state hands one iteration over (the twelve winners alone end with
            # loop_host == 1: test_zeroed_block_maxima_keep_the_loop_on_the_device); each group
            # of more than MAX_CAND tied candidates must hand over at least once more
            assert stats['loop_host'] >= 3, stats
            # (12 untied winners, then every selection of a group but its last is tied)
            assert stats['tie_passes'] >= sum(n - 1 for n, _ in TIES), stats


# ---- i. table upkeep -----------------------------------------------------------------------------
UPKEEP_KINDS = 211


def upkeep_corpus():
    """4088 two-token words p_k q_k of 211 kinds (8176 tokens: with 16 more the cold table's
    sizing bound is 8192 and its capacity 16 384, half full of the 4298 distinct pairs), in an
    order in which no two words follow each other twice: walks 0, d, 2 d .. mod 211 for
    d = 1, 2, ...  Every kind merges with W 19 or 20, and every boundary q_j p_k then becomes
    c_j p_k or q_j c_k, and c_j c_k: three claims each, 12 472 in all, past 3/4 of the capacity
    (12 288) some eight merges before the last.  (No corpus can do much better: a table sized
    for n tokens starts at most half full, and a merge of W sites claims at most 2 W new pairs
    while it takes W tokens away.)"""
    K, words = UPKEEP_KINDS, 4088
    seq = []
    d = 1
    while len(seq) < words:
        seq += [(i * d) % K for i in range(K)]
        d += 1
    seq = np.array(seq[:words])
    ids = np.empty(2 * words, np.int32)
    ids[0::2] = HOT + 2 * seq
    ids[1::2] = HOT + 2 * seq + 1
    return [ids], [1] * (HOT + 2 * K)


def run_upkeep():
    samples, len16 = upkeep_corpus()
    with Run(samples, len16) as r:
        per_batch = []
        for _ in range(2 * UPKEEP_KINDS // 8):
            n = r.batch(0, 8, 'loop')
            per_batch.append((r.e.stats()['cold_rebuilds'], r.in_state[-1]))
            if n < 8:
                break
        return r.merges, r.st.samples(), r.e.stats(), per_batch, r.maintained, r.checks


@gpu
def test_cold_table_is_rebuilt_from_itself(monkeypatch):
    monkeypatch.delenv('BPE_COLD_REBUILD', raising=False)
    merges, final, stats, per_batch, maintained, checks = run_upkeep()
    print(stats, per_batch)
    assert len(merges) == UPKEEP_KINDS
    assert stats['cold_rebuilds'] >= 1, stats
    # the tables were checked right after the rebuild (the batch it fell into ended maintained)
    first = next(i for i, (n, _) in enumerate(per_batch) if n >= 1)
    assert per_batch[first][1], per_batch
    assert maintained >= checks - 1
    monkeypatch.setenv('BPE_COLD_REBUILD', '0')
    merges0, final0, stats0, per_batch0, _, _ = run_upkeep()
    print(stats0, per_batch0)
    assert merges0 == merges and final0 == final
    assert stats0['cold_rebuilds'] == 0 and stats0['exact_passes'] > stats['exact_passes'], (stats, stats0)


# ---- j. transitions ------------------------------------------------------------------------------
def transition_corpus():
    rng = np.random.default_rng(10)
    return [rng.integers(HOT, HOT + 30, size=n).astype(np.int32) for n in (60_000, 40_000)], [1] * (HOT + 30)


def t_host_merge(r):
    r.batch(0, 1, 'host')


def t_replay(r, count_after):
    (a, b, W), = w = r.st.merge_until(0, 2, 1)
    got = r.e.apply_merges([(a, b, r.e.num_tokens())], count_after=count_after)
    assert [int(x) for x in got] == [W]
    r.merges += w
    r.check()


def t_add_sample(r):
    new = r.st.ids[100:700].copy()
    r.e.add_sample(new)
    r.st.ids = np.concatenate([r.st.ids[:r.st.off[-1]], new])
    r.st.off = np.concatenate([r.st.off, [r.st.off[-1] + len(new)]]).astype(np.int64)
    r.check()


def t_index_merge(r):
    w = r.st.merge_until(0, 2, 1)
    r.e.set_mode('incremental')
    assert r.e.merge_until(0, 2, 1) == w
    r.e.set_mode('stream')
    r.merges += w
    r.check()


def t_recount(r):
    r.e.recount()
    r.check()


TRANSITIONS = {
    'host_merge': t_host_merge,
    'replay_apply_only': lambda r: t_replay(r, False),
    'replay_counting': lambda r: t_replay(r, True),
    'add_sample': t_add_sample,
    'index_merge': t_index_merge,
    'recount': t_recount,
}


@gpu
@pytest.mark.parametrize('name', list(TRANSITIONS))
def test_transition_between_maintained_batches(name):
    """Each transition keeps the tables exact or drops the state (check() tells which, and checks
    the tables if they are kept); after re-entry they are exact again."""
    samples, len16 = transition_corpus()
    with Run(samples, len16) as r:
        r.batch(0, 8, 'loop')
        assert r.in_state[-1], 'the state was not entered'
        TRANSITIONS[name](r)
        kept = r.in_state[-1]
        r.batch(0, 8, 'loop')
        assert r.in_state[-1], ('no re-entry', r.in_state)
        TRANSITIONS[name](r)
        r.batch(0, 40, 'loop')
        print(name, 'kept' if kept else 'dropped', r.in_state, r.e.stats())
        assert r.in_state[-1] and r.maintained >= 3, r.in_state


@gpu
def test_compaction_between_maintained_batches():
    """1.1 M tokens (compaction needs 2^20 slots): two planted pairs enter the state, the third
    merge kills more than 1 % of the slots, and the next call compacts."""
    rng = np.random.default_rng(14)
    buf = rng.integers(HOT, HOT + 60, size=1_100_000).astype(np.int32)
    p, q, r_, s, h1, h2 = (HOT + 60 + i for i in range(6))
    sites = [(p, q)] * 16_000 + [(r_, s)] * 15_000 + [(h1, h2)] * 14_000
    cells = rng.permutation(len(buf) // 4 - 2)[:len(sites)] + 1
    for (x, y), c in zip(sites, cells):
        buf[4 * c + 1:4 * c + 3] = [x, y]
    with Run([buf, buf[:999].copy()], [1] * (HOT + 66)) as r:
        r.run([(0, 3), (0, 8), (0, 8)], 'loop')
        stats = r.e.stats()
        print(r.merges, r.in_state, stats)
        assert [m[:2] for m in r.merges[:3]] == [(p, q), (r_, s), (h1, h2)], r.merges[:3]
        assert stats['compactions'] >= 1, stats
        assert r.maintained == r.checks == 3, r.in_state


# ---- k. MODE_FUSED -------------------------------------------------------------------------------
@pytest.fixture
def fused(monkeypatch):
    """BPE_FUSED=1: the maintained state's fall-back form (a full hot recount with the cold
    refresh riding along); read when the engine is created."""
    monkeypatch.setenv('BPE_FUSED', '1')


@gpu
@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('seed', [1, 3])
def test_fused_random_all_cold(fused, seed, mode):
    run_random(seed, mode, 8)


@gpu
@pytest.mark.parametrize('mode', MODES)
def test_fused_placed_runs_chains_and_boundaries(fused, mode):
    run_placed_runs(mode)


@gpu
@pytest.mark.parametrize('mode', MODES)
def test_fused_placed_sites_beyond_emptied_chunks(fused, mode):
    run_placed_empties(mode)


@gpu
@pytest.mark.parametrize('mode', MODES)
def test_fused_cold_xx_runs_of_every_length(fused, mode):
    run_xx_runs(mode)


@gpu
@pytest.mark.parametrize('mode', MODES)
def test_fused_pairs_among_a_b_and_c(fused, mode):
    run_patterns(321, mode)


@gpu
def test_fused_passes_are_counted(fused):
    """(the knob took: the maintained merges ran as MODE_FUSED passes, none as MODE_INCR)"""
    samples, len16, _ = pattern_corpus(320)
    with Run(samples, len16) as r:
        r.run([(0, 8)], 'loop')
        stats = r.e.stats()
        assert stats['fused_passes'] >= 6 and stats['incr_launches'] == 0, stats
        assert r.maintained == 1


# ---- l. the vocabulary's end ---------------------------------------------------------------------
def vocab_end_corpus():
    rng = np.random.default_rng(55)
    ids = np.array([55_000, 55_001, 55_100, 55_255, 55_256, 55_287, 55_288, 55_289])
    return [rng.choice(ids, size=n).astype(np.int32) for n in (2500, 1500)], [1] * 55_290


@gpu
@pytest.mark.parametrize('mode', MODES)
def test_vocabulary_end(mode):
    """55 290 registered tokens: exactly six merges succeed (ids 55 290 .. 55 295); the next fails
    with BPE_ERR_VOCAB and leaves the corpus and the tables as they were.  'loop': four merges,
    then a call for five more, so that the device batch is cut to the two ids left (the loop's
    BPE_MAX_VOCAB - size clamp) and the third fails on the host path."""
    import ctypes
    samples, len16 = vocab_end_corpus()
    with Run(samples, len16, extra=64) as r:
        assert len(OracleState(*flat(samples), len16, len(len16), extra=64).merge_until(0, 2, 10)) == 10
        if mode == 'loop':
            r.run([(0, 4)], mode)
            assert len(r.merges) == 4 and r.in_state[-1]
            w = r.st.merge_until(0, 2, 2)
            out = np.zeros(3 * 8, np.int64)
            n = ctypes.c_int64(-1)
            rc = pkg.lib().bpe_merge_until(r.e._ctx, 0, 2, 5, out.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)),
                                           8, ctypes.byref(n))
            assert rc == pkg.ERR_VOCAB, (rc, pkg.last_error())
            # the two that fit were made, and are the oracle's
            assert [tuple(int(v) for v in out[3 * i:3 * i + 3]) for i in range(2)] == w
            r.merges += w
        else:
            r.run([(0, 6)], mode)
        assert len(r.merges) == 6 and r.e.num_tokens() == pkg.MAX_VOCAB
        r.check()
        assert r.in_state[-1]
        with pytest.raises(pkg.BpeError) as err:
            if mode == 'loop':
                r.e.merge_until(0, 2, 1)
            else:
                a, b, W = r.e.find_next_merge(0, 2)
                assert (a, b, W) == r.st.find_next_merge(0, 2)
                r.e.apply_merge(a, b, pkg.MAX_VOCAB)
        assert err.value.code == pkg.ERR_VOCAB
        r.check()
        a, b, W = r.st.find_next_merge(0, 2)
        with pytest.raises(pkg.BpeError) as err:
            r.e.apply_merge(a, b, pkg.MAX_VOCAB)
        assert err.value.code == pkg.ERR_VOCAB
        r.check()
        assert r.in_state[-1] and r.e.samples() == r.st.samples()
        assert r.e.num_tokens() == pkg.MAX_VOCAB
